"""Shared by tests/test_gpu_ensemble.py: the f64 restatement of csrc/ensemble.hip's network, its
cases, and a small REDQPolicy over an ensemble the kernel takes."""
import numpy as np
import torch

from tests.gail_common import worst_ratio  # noqa: F401

# (b, D, A, H, E): Din = 4, 23, 8, 393 -- every K tail; one row, a short tile, a tile plus one
# row, three tiles; the obs -> act crossing at aligned and unaligned columns; one member, several
CASES = [(1, 3, 1, 128, 1), (31, 17, 6, 256, 2), (33, 5, 3, 128, 3), (65, 376, 17, 256, 2)]
WALK = (1000, 17, 6, 256, 10)  # forward only: more tiles per member than workgroups walk at once


def make(b, D, A, H, E, seed=0):
    """(params, obs, act) as f64 seeded normal draws: params in EnsembleLinear's layout, w1
    [E, D + A, H], b1 [E, 1, H], w2 [E, H, H], b2 [E, 1, H], w3 [E, H, 1], b3 [E, 1, 1], the
    weights scaled by 1 / sqrt(fan-in)."""
    g = torch.Generator().manual_seed(seed + 1000 * b + D)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    params = [n(E, D + A, H) / (D + A) ** 0.5, n(E, 1, H), n(E, H, H) / H ** 0.5, n(E, 1, H),
              n(E, H, 1) / H ** 0.5, n(E, 1, 1)]
    return params, n(b, D), n(b, A)


def forward(params, obs, act, dtype=torch.float64):
    """q [E, b] in ``dtype``: EnsembleLinear's matmul + bias lines over the concatenated rows."""
    w1, b1, w2, b2, w3, b3 = (p.to(dtype) for p in params)
    x = torch.cat([obs, act], 1).to(dtype)
    h1 = torch.relu(torch.matmul(x, w1) + b1)
    h2 = torch.relu(torch.matmul(h1, w2) + b2)
    return (torch.matmul(h2, w3) + b3).squeeze(-1)


# -- a small REDQPolicy: 4 envs x 40 steps, obs 17 / act 6, hidden (128, 128), 3 members, subset 2
N_ENV, T, D, A, HIDDEN, MEMBERS, SUBSET, BATCH, SEED = 4, 40, 17, 6, (128, 128), 3, 2, 64, 11


def make_critics(dev, hidden=HIDDEN, activation=torch.nn.ReLU):
    from tianshou_amd.utils.net import Critic, EnsembleLinear, Net

    def linear(x, y):
        return EnsembleLinear(MEMBERS, x, y)

    return Critic(Net(D, A, hidden_sizes=hidden, activation=activation, concat=True, device=dev,
                      linear_layer=linear), device=dev, linear_layer=linear,
                  flatten_input=False).to(dev)


def make_policy(dev, fused_ensemble):
    """The policy (SGD on both networks: parameter changes are linear in the gradients) and a
    filled buffer, from seed SEED.  Rewards are 8 + N(0, 1) while the freshly initialised
    target min Q - alpha log_prob is O(1), so no return sits near zero, where a relative bound
    on rew + gamma target would measure cancellation and not the target."""
    from tianshou_amd.data import Batch, VectorReplayBuffer
    from tianshou_amd.policy import REDQPolicy
    from tianshou_amd.utils.net import ActorProb, Net
    torch.manual_seed(SEED)
    actor = ActorProb(Net(D, hidden_sizes=(32, 32), device=dev), (A,), device=dev, unbounded=True,
                      conditioned_sigma=True).to(dev)
    critics = make_critics(dev)
    policy = REDQPolicy(actor, torch.optim.SGD(actor.parameters(), lr=1e-2), critics,
                        torch.optim.SGD(critics.parameters(), lr=1e-2), ensemble_size=MEMBERS,
                        subset_size=SUBSET, actor_delay=2, action_scaling=False).to(dev)
    policy.fused_ensemble = fused_ensemble
    policy.train()
    rng, buf = np.random.default_rng(SEED), VectorReplayBuffer(N_ENV * T, N_ENV, device=dev)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    for t in range(T):
        buf.add(Batch(obs=f32(N_ENV, D), act=np.tanh(f32(N_ENV, A)), rew=8 + f32(N_ENV),
                      terminated=rng.random(N_ENV) < 0.05, truncated=np.zeros(N_ENV, bool),
                      obs_next=f32(N_ENV, D)), buffer_ids=np.arange(N_ENV))
    return policy, buf
