"""TD3BCPolicy (tianshou/policy/imitation/td3_bc.py:11-107): TD3 with a behaviour-cloning term
in the actor loss, on TD3Policy's device path (policy/td3.py), trained from a fixed buffer by
OfflineTrainer (trainer/base.py).

The critics' step is TD3's.  The actor loss -lmbda * mean(Q) + mse(act, data_act) with lmbda =
alpha / mean|Q| held constant is ``tsrl_td3bc_actor_loss_fwd_bwd`` (csrc/offline_cont.hip): the
loss and both gradients in one launch up to 256 rows, two beyond, and no host read.  ``_cnt``,
``_last`` and ``update_actor_freq`` behave as TD3's, and an update replays from one of TD3's two
HIP graphs per shape.  ``fused = False`` is the reference's op sequence.
"""
from typing import Any, Optional

import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.exploration import BaseNoise, GaussianNoise
from tianshou_amd.policy.ddpg import q_mse_loss
from tianshou_amd.policy.flat_learn import KernelGradLoss, _partials
from tianshou_amd.policy.td3 import TD3Policy


class _TD3BCActorLoss(KernelGradLoss):
    """td3_bc.py:91-96 as tsrl_td3bc_actor_loss_fwd_bwd.  args: (data_act [b, A] f32, alpha,
    loss [1]).  The output is the handle to call backward on, towards q [b] and act [b, A]."""

    @staticmethod
    def forward(ctx, args, q, act):
        data_act, alpha, loss = args
        x = q.detach().to(torch.float32).contiguous().view(-1)
        a = act.detach().to(torch.float32).contiguous()
        b, dev = x.numel(), x.device
        if a.dim() != 2 or a.shape[0] != b or data_act.shape != a.shape or loss.numel() != 1:
            raise ValueError(f"_TD3BCActorLoss: q needs {b} elements, act and data_act one "
                             f"[{b}, A] shape, loss one element")
        grads = [torch.empty_like(x), torch.empty_like(a)]
        _C.check(_C.lib().tsrl_td3bc_actor_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(a), _C.ptr(data_act, torch.float32), float(alpha), b, a.shape[1],
            _C.ptr(grads[0]), _C.ptr(grads[1]), _C.ptr(_partials(b, 3, dev)),
            _C.ptr(loss, torch.float32), _C.stream_ptr(dev)), "tsrl_td3bc_actor_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q, act))
        return torch.empty((), dtype=torch.float32, device=dev)


def td3bc_actor_loss(q: torch.Tensor, act: torch.Tensor, data_act: torch.Tensor, alpha: float,
                     loss_out: torch.Tensor) -> torch.Tensor:
    """The backward handle of -lmbda * mean(q) + mse(act, data_act); the loss goes to
    ``loss_out`` (one f32 element)."""
    return _TD3BCActorLoss.apply((data_act, alpha, loss_out), q, act)


class TD3BCPolicy(TD3Policy):
    """Constructor arguments and defaults as the reference's (td3_bc.py:53-77)."""

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critic1: torch.nn.Module, critic1_optim: torch.optim.Optimizer,
                 critic2: torch.nn.Module, critic2_optim: torch.optim.Optimizer,
                 tau: float = 0.005, gamma: float = 0.99,
                 exploration_noise: Optional[BaseNoise] = GaussianNoise(sigma=0.1),
                 policy_noise: float = 0.2, update_actor_freq: int = 2,
                 noise_clip: float = 0.5, alpha: float = 2.5,
                 reward_normalization: bool = False, estimation_step: int = 1,
                 **kwargs: Any) -> None:
        super().__init__(actor, actor_optim, critic1, critic1_optim, critic2, critic2_optim, tau,
                         gamma, exploration_noise, policy_noise, update_actor_freq, noise_clip,
                         reward_normalization, estimation_step, **kwargs)
        self._alpha = alpha

    def _learn_torch(self, batch: Batch, do_actor: bool):
        """td3_bc.py:79-102 as written; returns (losses, per-row vector)."""
        td1, critic1_loss = self._mse_optimizer(batch, self.critic1, self.critic1_optim)
        td2, critic2_loss = self._mse_optimizer(batch, self.critic2, self.critic2_optim)
        losses = [critic1_loss.detach(), critic2_loss.detach()]
        if do_actor:
            act = self(batch, eps=0.0).act
            q_value = self.critic1(batch.obs, act)
            lmbda = self._alpha / q_value.abs().mean().detach()
            actor_loss = -lmbda * q_value.mean() + F.mse_loss(
                act, torch.as_tensor(batch.act, device=act.device).to(act.dtype))
            self.actor_optim.zero_grad()
            actor_loss.backward()
            losses.append(actor_loss.detach())
            self.actor_optim.step()
            self.sync_weight()
        return torch.stack(losses), ((td1 + td2) / 2.0).detach()

    def _step(self, fas, obs, act, returns, weight, do_actor: bool, td_out: torch.Tensor,
              loss_out: torch.Tensor) -> None:
        """DDPGPolicy._step with the actor part on the TD3+BC loss kernel."""
        names = self._critic_names
        qs = [getattr(self, name)(obs, act).flatten() for name in names]
        handle, _, _ = q_mse_loss(qs, returns, weight, td_out, loss_out[:2])
        self._backward_step(handle, names, fas)
        if not do_actor:
            return
        a, _ = self.actor(obs, state=None, info=Batch())
        q = self.critic1(obs, a).flatten()
        handle = td3bc_actor_loss(q, a, act, self._alpha, loss_out[2:3])
        self._backward_step(handle, ("actor",), fas)
        self.sync_weight()
