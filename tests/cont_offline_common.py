"""Shared by tests/test_cont_offline_host.py and tests/test_gpu_cont_offline.py: the three loss
formulas of tianshou/policy/imitation/cql.py and td3_bc.py on torch f64 with autograd -- the
judge of the fused kernels' analytic gradients -- and the policies of
tests/golden/cont_offline.npz (tools/gen_goldens.py gen_cont_offline: the reference on CPU)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.offline_common import assert_state, state  # noqa: F401  (re-exported)


def _leaf(x):
    return torch.as_tensor(x, dtype=torch.float64).requires_grad_()


def cql_ref(q1, q2, target, v1, v2, log_pi, log_alpha, T, w, thr, amin, amax, A, lagrange,
            dtype=torch.float64):
    """cql.py:198-260: (critic1, critic2, multiplier loss, cql_alpha), the gradients towards q1,
    q2, v1, v2 of each critic's own loss, and the multiplier's gradient.  v: [3, n]."""
    leaves = [torch.as_tensor(x, dtype=dtype).requires_grad_() for x in (q1, q2, v1, v2)]
    la = torch.as_tensor(log_alpha, dtype=dtype).requires_grad_()
    t, lp = torch.as_tensor(target, dtype=dtype), torch.as_tensor(log_pi, dtype=dtype)
    a = torch.clamp(la.exp(), amin, amax) if lagrange else torch.ones((), dtype=dtype)
    losses, cqls = [], []
    for q, v in zip(leaves[:2], leaves[2:]):
        cat = torch.stack([v[0] - np.log(0.5 ** A), v[1] - lp[0], v[2] - lp[1]], 1)
        cql = torch.logsumexp(cat / T, dim=1).mean() * w * T - q.mean() * w
        cqls.append(a * (cql - thr) if lagrange else cql)
        losses.append(F.mse_loss(q, t) + cqls[-1])
    alpha_loss = -(cqls[0] + cqls[1]) * 0.5
    g_la = torch.autograd.grad(alpha_loss, la, retain_graph=True)[0] if lagrange else None
    (losses[0] + losses[1]).backward()
    out = [x.detach().numpy() for x in (*losses, alpha_loss, a)]
    return out, [x.grad.numpy() for x in leaves], None if g_la is None else g_la.numpy()


def td3bc_ref(q, act, data_act, alpha):
    """td3_bc.py:91-96: loss, grad_q, grad_act."""
    q, a = _leaf(q), _leaf(act)
    lmbda = alpha / q.abs().mean().detach()
    loss = -lmbda * q.mean() + F.mse_loss(a, torch.as_tensor(data_act, dtype=torch.float64))
    loss.backward()
    return loss.item(), q.grad.numpy(), a.grad.numpy()


# -- the recording ------------------------------------------------------------------------------
def recording(golden_dir):
    z = np.load(os.path.join(golden_dir, "cont_offline.npz"))
    return z, json.loads(str(z["cfg"]))


def make_policy(z, cfg, tag, dev="cpu", **attrs):
    """The variant's policy over this package's networks, the recorded initial state_dict (the
    reference's checkpoint) loaded with strict=True."""
    from tianshou_amd import policy as P
    from tianshou_amd.utils.net import Actor, ActorProb, Critic, Net
    v, D, A, H = cfg["variants"][tag], cfg["D"], cfg["A"], cfg["hidden"]
    critics = [Critic(Net(D, A, hidden_sizes=(H, H), concat=True, device=dev), device=dev)
               for _ in range(2)]
    if v["kind"] == "td3bc":
        actor = Actor(Net(D, hidden_sizes=(H, H), device=dev), (A,), device=dev)
    else:
        actor = ActorProb(Net(D, hidden_sizes=(H, H), device=dev), (A,), device=dev,
                          unbounded=True, conditioned_sigma=True)
    nets = [m.to(dev) for m in (actor, *critics)]
    opt = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in nets]
    args = (nets[0], opt[0], nets[1], opt[1], nets[2], opt[2])
    if v["kind"] == "td3bc":
        policy = P.TD3BCPolicy(*args, tau=cfg["tau"], gamma=cfg["gamma"], exploration_noise=None,
                               action_scaling=False, **v["kw"])
    else:
        alpha = 0.2
        if v["auto"]:
            la = torch.zeros(1, requires_grad=True, device=dev)
            alpha = (-float(A), la, torch.optim.Adam([la], lr=cfg["alpha_lr"]))
        policy = P.CQLPolicy(*args, cql_alpha_lr=cfg["cql_alpha_lr"], tau=cfg["tau"],
                             gamma=cfg["gamma"], alpha=alpha, num_repeat_actions=cfg["R"],
                             action_scaling=False, device=dev, **v["kw"])
    policy.load_state_dict(state(z, f"{tag}_init_sd_"), strict=True)
    policy.to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy


def feed_draws(policy, z, tag, updates):
    """Replace the policy's draw methods by the recorded draws, in the order they were made."""
    def feeder(kind):
        it = (z[f"{tag}_u{u}_{kind}{i}"] for u in range(updates)
              for i in range(int(z[f"{tag}_u{u}_n_{kind}"])))

        def recorded(shape, device):
            d = next(it)
            assert tuple(shape) == d.shape, (kind, tuple(shape), d.shape)
            return torch.as_tensor(d, device=device)
        return recorded
    policy._rsample_noise, policy._cql_uniform, policy._smoothing_noise = \
        feeder("normal"), feeder("uniform"), feeder("randn")


def check_update(policy, z, tag, u, res, loss_rtol):
    """One update's losses (the reference's keys and order), parameters (the Adam bound, rtol
    1e-5 / atol 1e-6) and the temperature and multiplier."""
    q = f"{tag}_u{u}_"
    assert list(res) == json.loads(str(z[tag + "_loss_keys"]))
    np.testing.assert_allclose(list(res.values()), z[q + "losses"], rtol=loss_rtol, atol=1e-6,
                               err_msg=q)
    assert_state(policy, z, q + "sd_", q)
    for key, attr in (("cql_log_alpha", "cql_log_alpha"), ("log_alpha", "_log_alpha")):
        if q + key in z.files:
            np.testing.assert_allclose(getattr(policy, attr).detach().cpu().numpy(), z[q + key],
                                       rtol=1e-5, atol=1e-6, err_msg=q + key)
