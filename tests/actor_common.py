"""Shared by tests/test_actor_ref.py (CPU) and tests/test_gpu_actor_ref.py (GPU): the actor of
tests/test_gpu_policy_act.py::_actor (orthogonal init, 0.01-scaled mu head, every parameter
perturbed by 0.05 N(0,1) so biases and log-std are non-trivial) and its weights as f64 arrays
for oracle/actor_ref.py."""
import numpy as np
import torch

# (D, A, n) of the shape-edge cases of the policy.hip actor (and the D, A of its f32 headroom)
SHAPE_CASES = [
    (1, 1, 1),        # one row, one column, one action: every padding path at once
    (3, 2, 31),       # D < 4: a single ragged group; n < 32
    (5, 2, 33),       # D % 4 == 1; two workgroups, the second with one row
    (16, 31, 32),     # exactly one padded K block; odd A (last noise pair half used)
    (17, 6, 70),      # config 2's width: scalar row path
    (33, 32, 70),     # A = AMAX
    (48, 17, 70),     # G = 6 < 8: two of the 8 waves get no K-groups
    (376, 17, 70),    # the headline width
    (1000, 32, 70),   # 15-16 groups per wave: three GB = 6 batches with a ragged tail
]
BOUND_CASE = (24, 17, 70)  # the FlatAdam-bound actor


def make_actor(D, A, dev, seed):
    from tianshou_amd.utils.models import get_actor_critic, init_actor_critic
    torch.manual_seed(seed)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    actor, critic = actor.to(dev), critic.to(dev)
    init_actor_critic(actor, critic)
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return actor, critic


def layer_arrays(layers):
    """(W1, b1, W2, b2, W3, b3, log_std) of a fused_act.match_actor() dict as f64 arrays."""
    def a(t):
        return t.detach().cpu().numpy().astype(np.float64)
    return (a(layers["w1"].weight), a(layers["w1"].bias), a(layers["w2"].weight),
            a(layers["w2"].bias), a(layers["w3"].weight), a(layers["w3"].bias),
            a(layers["sigma"]).reshape(-1))
