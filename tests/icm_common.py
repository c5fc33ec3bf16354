"""Shared by tests/test_gpu_icm.py and tests/test_icm_host.py: the curiosity head of
include/tsrl.h (csrc/icm.hip) restated in torch on the CPU (f64 reference, or f32: the reference
formulation's own error), a seeded ``make``, the case table, small ICMPolicy builders and the
ICM phase of ``ICMPolicy.update`` in f64.  Parameter lists follow parameters(): forward model
(W1, b1, W2, b2), inverse model (W1, b1, W2, b2)."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from tests.gail_common import split, worst_ratio  # noqa: F401

# (M, W, A): a single row / one row short of a 32-row tile / one row past it, widest A / one row
# past a 64-row tile / more tiles than workgroups
CASES = [(1, 64, 2), (31, 128, 3), (33, 128, 32), (65, 128, 2), (64 * 256 + 1, 64, 6)]
MIN_Z = 1e-4


def hidden(p, phi1, phi2, act):
    """The two hidden pre-activations z_f, z_i."""
    W = phi1.shape[1]
    z_f = phi1 @ p[0][:, :W].T + p[0][:, W:].T[act] + p[1]
    return z_f, torch.cat([phi1, phi2], 1) @ p[4].T + p[5]


def head(p, phi1, phi2, act, dtype=torch.float64):
    """(mse_loss, act_hat) of discrete.py:440-449 on the features, computed in ``dtype``."""
    p, phi1, phi2 = [t.to(dtype) for t in p], phi1.to(dtype), phi2.to(dtype)
    z_f, z_i = hidden(p, phi1, phi2, act)
    e = torch.relu(z_f) @ p[2].T + p[3] - phi2
    return 0.5 * (e * e).sum(1), torch.relu(z_i) @ p[6].T + p[7]


def make(M, W, A, seed=0):
    """(params, phi1, phi2, act) in f64.  Rows with a hidden pre-activation below MIN_Z in
    magnitude are scaled by 1.5 until none is, so that an f32 evaluation cannot land on the
    other side of a ReLU."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k  # noqa: E731
    lin = lambda o, i: [r(o, i, k=i ** -0.5), r(o, k=0.1 * i ** -0.5)]  # noqa: E731
    params = lin(W, W + A) + lin(W, W) + lin(W, 2 * W) + lin(A, W)
    phi, act = r(M, 2 * W), torch.arange(M) % A
    low = lambda: torch.cat(hidden(params, phi[:, :W], phi[:, W:], act), 1).abs().min(1)[0]  # noqa: E731
    for _ in range(20):
        phi[low() < MIN_Z] *= 1.5
    assert float(low().min()) >= MIN_Z
    return params, phi[:, :W].contiguous(), phi[:, W:].contiguous(), act


def step(params, phi1, phi2, act, w, lr_scale, dtype=torch.float64):
    """icm.py:106-114 in ``dtype``: ((loss, forward, inverse), the eight gradients flat, d_phi1,
    d_phi2) by autograd; phi2 is not detached as the forward model's target."""
    p = [t.to(dtype).requires_grad_() for t in params]
    f1, f2 = (t.to(dtype).requires_grad_() for t in (phi1, phi2))
    mse, act_hat = head(p, f1, f2, act, dtype)
    inverse, forward = F.cross_entropy(act_hat, act).mean(), mse.mean()
    loss = ((1 - w) * inverse + w * forward) * lr_scale
    *gp, d1, d2 = torch.autograd.grad(loss, p + [f1, f2])
    return torch.stack([loss, forward, inverse]).detach(), \
        torch.cat([t.reshape(-1) for t in gp]), d1, d2


# -- small ICMPolicy runs: 200 transitions, ICM over DQN (CartPole's shape, W 128) and over PPO --
KINDS = {"dqn": dict(D=4, A=2, W=128, sample=64, kw={}),
         "ppo": dict(D=8, A=6, W=64, sample=0, kw=dict(batch_size=100, repeat=1))}
E, T, LR, LR_SCALE, REW_SCALE, FWD_W = 8, 25, 1e-3, 0.5, 0.01, 0.2


def rows(kind, seed=5):
    c, rng = KINDS[kind], np.random.RandomState(seed)
    f = lambda *s: rng.randn(*s).astype(np.float32)  # noqa: E731
    return dict(obs=f(T, E, c["D"]), act=rng.randint(0, c["A"], (T, E)), rew=rng.randn(T, E),
                terminated=rng.rand(T, E) < 0.1, obs_next=f(T, E, c["D"]))


def icm_model(kind, dev, hidden_sizes=None, activation=torch.nn.ReLU, W=None, A=None, seed=1):
    from tianshou_amd.utils.net import MLP, IntrinsicCuriosityModule
    c = KINDS[kind]
    W, A = W or c["W"], A or c["A"]
    torch.manual_seed(seed)
    model = IntrinsicCuriosityModule(MLP(c["D"], output_dim=W, hidden_sizes=(32,), device=dev),
                                     W, A, hidden_sizes=hidden_sizes or (W,), device=dev)
    if activation is not torch.nn.ReLU:
        model.forward_model.model[1] = model.inverse_model.model[1] = activation()
    return model.to(dev)


def wrap(inner, model, fused, optim=None, reward_scale=REW_SCALE):
    from tianshou_amd.policy import ICMPolicy
    optim = optim or torch.optim.Adam(model.parameters(), lr=LR)
    return ICMPolicy(inner, model, optim, LR_SCALE, reward_scale, FWD_W, fused=fused)


def phase_f64(model, obs, act, obs_next):
    """process_fn's forward and learn()'s ICM step in f64 on the CPU, Adam with torch's defaults:
    ((loss, forward, inverse), mse_loss, the flat first gradient, the flat parameters after)."""
    m = copy.deepcopy(model).cpu().double()
    feat, fwd, inv = m.feature_net.model, m.forward_model.model, m.inverse_model.model
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    obs, obs_next, act = (torch.as_tensor(np.asarray(x)) for x in (obs, obs_next, act))
    phi1, phi2 = feat(obs.double()), feat(obs_next.double())
    e = fwd(torch.cat([phi1, F.one_hot(act.long(), m.action_dim)], 1)) - phi2
    mse = 0.5 * (e * e).sum(1)
    inverse = F.cross_entropy(inv(torch.cat([phi1, phi2], 1)), act.long())
    forward = mse.mean()
    loss = ((1 - FWD_W) * inverse + FWD_W * forward) * LR_SCALE
    loss.backward()
    flat = lambda ts: torch.cat([t.detach().reshape(-1).clone() for t in ts])  # noqa: E731
    grad = flat(p.grad for p in m.parameters())
    opt.step()
    return [float(x.detach()) for x in (loss, forward, inverse)], mse.detach(), grad, \
        flat(m.parameters())


def keep_mask(model, grad):
    """Adam's first step is sign-like: elements whose first gradient is tiny but not zero are
    left out (tests/test_gpu_gail.py).  An exactly zero gradient (a hidden unit no row activates)
    stays in: every leg leaves that element where it was."""
    return torch.cat([(g == 0) | (g.abs() >= 1e-6 * g.abs().max())
                      for g in split(grad, list(model.parameters()))])
