"""Shared by tests/test_gpu_gail.py and tests/test_gail_host.py: the GAIL discriminator step of
include/tsrl.h restated in torch on the CPU (f64 reference, or f32: the reference formulation's
own error), a seeded ``make``, the case table and a small GAILPolicy builder.  Flat vectors
follow disc_net.parameters(): W1, b1, W2, b2, w3, b3."""
import numpy as np
import torch
import torch.nn.functional as F

# (m_pi, m_exp, D, A); the reward tests use (n = m_pi, D, A).  Single row and tiny widths / one
# row short of a tile, a chunk across D / exact tile, D + A = 64 / one row past a tile, D + A =
# 393: the second panel / more tiles than workgroups
CASES = [(1, 1, 3, 1), (63, 65, 33, 17), (64, 64, 60, 4), (65, 130, 376, 17),
         (64 * 256 + 1, 64, 17, 6)]
N_EXPERT = 50
MIN_D = 1e-3


def logits(params, X):
    W1, b1, W2, b2, w3, b3 = params
    return (torch.tanh(torch.tanh(X @ W1.T + b1) @ W2.T + b2) @ w3.T + b3).flatten()


def make(m_pi, m_exp, D, A, seed=0):
    """(params, policy obs / act, expert obs / act [N_EXPERT rows], expert draws [m_exp] with
    replacement), f64.  Rows whose |d| is below MIN_D are scaled by 1.5 until none is, so that
    an f32 evaluation cannot land on the other side of 0."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k  # noqa: E731
    K = D + A
    params = [r(64, K, k=K ** -0.5), r(64, k=0.1), r(64, 64, k=0.125), r(64, k=0.1),
              r(1, 64, k=0.5), r(1, k=0.1)]
    xs = [r(m_pi, K), r(N_EXPERT, K)]
    for x in xs:
        for _ in range(20):
            x[logits(params, x).abs() < MIN_D] *= 1.5
        assert float(logits(params, x).abs().min()) >= MIN_D
    idx = torch.randint(N_EXPERT, (m_exp,), generator=g)
    return params, xs[0][:, :D], xs[0][:, D:], xs[1][:, :D], xs[1][:, D:], idx


def reward(params, obs, act, dtype=torch.float64):
    p = [t.to(dtype) for t in params]
    return -F.logsigmoid(-logits(p, torch.cat([obs, act], 1).to(dtype)))


def disc_step(params, x_pi, x_exp, dtype=torch.float64):
    """gail.py:130-141 on rows x = cat(obs, act): (loss, acc_pi, acc_exp, flat autograd
    gradient), computed in ``dtype``."""
    p = [t.to(dtype).requires_grad_() for t in params]
    d_pi, d_exp = logits(p, x_pi.to(dtype)), logits(p, x_exp.to(dtype))
    loss = -F.logsigmoid(-d_pi).mean() + -F.logsigmoid(d_exp).mean()
    grad = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss, p)])
    return loss.detach(), (d_pi < 0).to(dtype).mean(), (d_exp > 0).to(dtype).mean(), grad


def split(flat, params):
    out, o = [], 0
    for p in params:
        out.append(flat[o:o + p.numel()])
        o += p.numel()
    return out


def worst_ratio(got, ref32, ref64, blocks=None):
    """Worst (error of got) / max(error of ref32, floor / 4) over the blocks and over max-abs
    and 2-norm; floor = 2^-23 ||ref64||_2, f32's own resolution (tests/test_gpu_fvp.py)."""
    got, ref32, ref64 = (torch.as_tensor(t, dtype=torch.float64).reshape(-1)
                         for t in (got, ref32, ref64))
    floor = 2.0 ** -23 * float(ref64.norm())
    trip = zip(*(split(t, blocks) for t in (got, ref32, ref64))) if blocks else \
        [(got, ref32, ref64)]
    worst = 0.0
    for g, t, r in trip:
        for norm in (lambda d: float(d.abs().max()), lambda d: float(d.norm())):
            worst = max(worst, norm(g - r) / max(norm(t - r), floor / 4))
    return worst


# -- a small GAILPolicy: 8 envs x 40 steps, obs 17 / act 6 -------------------------------------
E, T, D, A, N_EXP_BUF = 8, 40, 17, 6, 500


def policy_data(seed=3):
    """Rollout and expert transitions as numpy arrays (f32 obs / act)."""
    rng = np.random.default_rng(seed)
    roll = dict(obs=rng.standard_normal((T, E, D)).astype(np.float32),
                act=rng.uniform(-1, 1, (T, E, A)).astype(np.float32),
                done=rng.random((T, E)) < 0.05)
    expert = dict(obs=rng.standard_normal((N_EXP_BUF, D)).astype(np.float32) + 0.5,
                  act=rng.uniform(-1, 1, (N_EXP_BUF, A)).astype(np.float32))
    return roll, expert


def make_policy(dev, fused, disc_update_num=4, activation=torch.nn.Tanh, hidden=64,
                concat=True, seed=0):
    """(policy, rollout buffer) with irl_gail.py's networks; the rollout buffer is None on the
    CPU (the buffer and PPO's own kernels live on the device)."""
    from tianshou_amd.data import Batch, ReplayBuffer, VectorReplayBuffer
    from tianshou_amd.policy import GAILPolicy
    from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_and_get_optim
    from tianshou_amd.utils.net import Critic, Net
    torch.manual_seed(seed)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    optim = init_and_get_optim(actor, critic, 3e-4)
    disc = Critic(Net((D,), action_shape=(A,), hidden_sizes=(hidden, hidden),
                      activation=activation, device=dev, concat=concat), device=dev).to(dev)
    disc_optim = torch.optim.Adam(disc.parameters(), lr=2.5e-5)
    roll, ex = policy_data()
    zeros = np.zeros(N_EXP_BUF)
    cuda = torch.device(dev).type == "cuda"
    expert = ReplayBuffer.from_data(ex["obs"], ex["act"], zeros, zeros > 0, zeros > 0, zeros > 0,
                                    ex["obs"]) if cuda else _HostExpert(ex)
    policy = GAILPolicy(actor, critic, optim, fixed_std_normal, expert, disc, disc_optim,
                        disc_update_num, fused=fused, action_scaling=False).to(dev)
    buf = None
    if cuda:
        buf = VectorReplayBuffer(E * T, E, device=dev)
        for t in range(T):
            nxt = roll["obs"][(t + 1) % T]
            buf.add(Batch(obs=roll["obs"][t], act=roll["act"][t], rew=np.zeros(E),
                          terminated=roll["done"][t], truncated=np.zeros(E, bool),
                          obs_next=nxt), buffer_ids=np.arange(E))
    return policy, buf


class _HostExpert:
    """The two calls GAILPolicy makes on its expert buffer, over host arrays."""

    def __init__(self, ex):
        self.ex = ex

    def sample(self, bsz):
        from tianshou_amd.data import Batch
        idx = np.random.choice(N_EXP_BUF, bsz)
        return Batch(obs=self.ex["obs"][idx], act=self.ex["act"][idx]), idx


def disc_phase_f64(params, obs, act, ex, n, num, lr=2.5e-5, first_grad=None):
    """The discriminator phase of GAILPolicy.learn in f64 (np.random: the permutation, then one
    expert draw per step; Adam with torch's defaults): (losses, acc_pis, acc_exps, params)."""
    from tianshou_amd.data.batch import split_indices
    p = [t.double().clone().requires_grad_() for t in params]
    opt = torch.optim.Adam(p, lr=lr)
    x = torch.cat([torch.as_tensor(obs), torch.as_tensor(act)], 1).double()
    xe = torch.cat([torch.as_tensor(ex["obs"]), torch.as_tensor(ex["act"])], 1).double()
    bsz, rows = n // num, []
    for part in split_indices(n, bsz, True, True):
        e = np.random.choice(N_EXP_BUF, bsz)
        loss, a_pi, a_exp, grad = disc_step([t.detach() for t in p], x[part], xe[e])
        if first_grad is not None and not rows:
            first_grad.append(grad)
        for t, g in zip(p, split(grad, p)):
            t.grad = g.view_as(t).clone()
        opt.step()
        rows.append((float(loss), float(a_pi), float(a_exp)))
    return (*(list(c) for c in zip(*rows)), [t.detach() for t in p])
