"""TD3Policy (tianshou/policy/modelfree/td3.py:52-134): twin critics, target policy smoothing
and a delayed actor step, on DDPGPolicy's device path (policy/ddpg.py).

Both critics' losses come from one ``tsrl_q_mse_fwd_bwd`` launch, the smoothing of
``_target_q`` is one ``tsrl_td3_smooth`` launch, and ``sync_weight`` covers all three networks
in one ``tsrl_soft_update`` launch.  An update replays from one of two HIP graphs per shape:
the critics alone, or the critics, the actor step and the soft update.  ``_cnt`` stays on the
host and ``_last`` is kept between actor steps, as in the reference.
"""
from copy import deepcopy
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.exploration import BaseNoise, GaussianNoise
from tianshou_amd.policy.ddpg import DDPGPolicy


def td3_smooth_device(act: torch.Tensor, noise: torch.Tensor, sigma: float, clip: float
                      ) -> torch.Tensor:
    """td3.py:101-104 as one launch, in place on a contiguous f32 ``act``:
    act += clamp(noise * sigma, -clip, clip), the clamp skipped when clip <= 0."""
    if noise.shape != act.shape:
        raise ValueError(f"td3_smooth_device: noise {tuple(noise.shape)} != act "
                         f"{tuple(act.shape)}")
    noise = noise.to(torch.float32).contiguous()
    _C.check(_C.lib().tsrl_td3_smooth(_C.ptr(act, torch.float32), _C.ptr(noise), float(sigma),
                                      float(clip), act.numel(), _C.ptr(act),
                                      _C.stream_ptr(act.device)), "tsrl_td3_smooth")
    return act


class TD3Policy(DDPGPolicy):
    """Constructor arguments and defaults as the reference's (td3.py:52-84); the device-path
    attributes are DDPGPolicy's."""

    _critic_names = ("critic1", "critic2")
    _sync_order = ("critic1", "critic2", "actor")  # td3.py:94-96

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critic1: torch.nn.Module, critic1_optim: torch.optim.Optimizer,
                 critic2: torch.nn.Module, critic2_optim: torch.optim.Optimizer,
                 tau: float = 0.005, gamma: float = 0.99,
                 exploration_noise: Optional[BaseNoise] = GaussianNoise(sigma=0.1),
                 policy_noise: float = 0.2, update_actor_freq: int = 2,
                 noise_clip: float = 0.5, reward_normalization: bool = False,
                 estimation_step: int = 1, **kwargs: Any) -> None:
        super().__init__(actor, actor_optim, None, None, tau, gamma, exploration_noise,
                         reward_normalization, estimation_step, **kwargs)
        self.critic1, self.critic1_old = critic1, deepcopy(critic1)
        self.critic1_old.eval()
        self.critic1_optim = critic1_optim
        self.critic2, self.critic2_old = critic2, deepcopy(critic2)
        self.critic2_old.eval()
        self.critic2_optim = critic2_optim
        self._policy_noise = policy_noise
        self._freq = update_actor_freq
        self._noise_clip = noise_clip
        self._cnt = 0
        self._last = 0

    def _smoothing_noise(self, shape, device) -> torch.Tensor:
        """The N(0, 1) draw of td3.py:101 (before the scaling by policy_noise)."""
        return torch.randn(size=shape, device=device)

    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """td3.py:98-109: min over the target critics at the smoothed target action."""
        obs_next = self._obs_next(buffer, indices)
        batch = Batch(obs_next=obs_next, info=Batch())
        act_ = self(batch, model="actor_old", input="obs_next").act
        noise = self._smoothing_noise(act_.shape, act_.device)
        if self.fused and act_.is_cuda and act_.dtype == torch.float32:
            act_ = td3_smooth_device(act_.contiguous(), noise, self._policy_noise,
                                     self._noise_clip)
        else:
            noise = noise * self._policy_noise
            if self._noise_clip > 0.0:
                noise = noise.clamp(-self._noise_clip, self._noise_clip)
            act_ += noise
        return torch.min(self.critic1_old(obs_next, act_), self.critic2_old(obs_next, act_))

    def _actor_step_due(self) -> bool:
        return self._cnt % self._freq == 0

    def _result(self, losses: List[float], did_actor: bool) -> Dict[str, float]:
        """td3.py:122-134."""
        if did_actor:
            self._last = losses[2]
        self._cnt += 1
        return {"loss/actor": self._last, "loss/critic1": losses[0], "loss/critic2": losses[1]}
