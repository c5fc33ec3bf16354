"""utils.net.ensemble_critic(learn=True) without a GPU: the torch lines, bit for bit."""
import torch

from tests import ensemble_common as ec
from tianshou_amd.utils.net import ensemble_critic


def test_learn_on_cpu_tensors_is_the_torch_lines():
    torch.manual_seed(5)
    critic = ec.make_critics("cpu")
    obs, dq = torch.randn(9, ec.D), torch.randn(ec.MEMBERS, 9, 1)
    grads = []
    for fn in (lambda a: ensemble_critic(critic, obs, a, learn=True), lambda a: critic(obs, a)):
        a = torch.randn(9, ec.A, generator=torch.Generator().manual_seed(1)).requires_grad_()
        q = fn(a)
        grads.append((q.detach(),) + torch.autograd.grad(q, [a, *critic.parameters()], dq))
    assert all(torch.equal(x, y) for x, y in zip(*grads))
