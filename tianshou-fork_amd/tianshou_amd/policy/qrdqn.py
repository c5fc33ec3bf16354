"""QRDQNPolicy (tianshou/policy/modelfree/qrdqn.py:12-97): quantile-regression DQN,
arXiv:1710.10044, on DQNPolicy's device path.

The network returns N quantile values per action, [b, A, N] (utils/net.py
``Net(num_atoms=N)``, utils/net_atari.py ``QRDQN``).  Acting and ``_target_q`` are
tsrl_dist_select (the mean over the quantiles, the greedy action, its row); learn() is
tsrl_qr_loss_fwd_bwd, which walks the N x N quantile pairs of a row out of LDS instead of
building the reference's [b, N, N] tensors.  ``fused = False`` runs the reference's op sequence
on torch, and so does learn() with more quantiles than the loss kernel takes
(``_C.DIST_MAX_N``).
"""
import warnings
from typing import Any, Optional

import numpy as np
import torch
import torch.nn.functional as F

from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.dqn import DQNPolicy
from tianshou_amd.policy.dqn_dist import DistDQNMixin, _QRLoss


class QRDQNPolicy(DistDQNMixin, DQNPolicy):
    """Constructor arguments, defaults, assertions and attributes as the reference's
    (qrdqn.py:35-56): ``tau_hat`` holds the quantile midpoints as a non-trainable [1, N, 1]
    parameter."""

    def __init__(self, model: torch.nn.Module, optim: torch.optim.Optimizer,
                 discount_factor: float = 0.99, num_quantiles: int = 200,
                 estimation_step: int = 1, target_update_freq: int = 0,
                 reward_normalization: bool = False, **kwargs: Any) -> None:
        super().__init__(model, optim, discount_factor, estimation_step, target_update_freq,
                         reward_normalization, **kwargs)
        assert num_quantiles > 1, "num_quantiles should be greater than 1"
        self._num_quantiles = num_quantiles
        tau = torch.linspace(0, 1, self._num_quantiles + 1)
        self.tau_hat = torch.nn.Parameter(((tau[:-1] + tau[1:]) / 2).view(1, -1, 1),
                                          requires_grad=False)
        warnings.filterwarnings("ignore", message="Using a target size")

    def _q_weights(self) -> Optional[torch.Tensor]:
        return None

    def _num_columns(self) -> int:
        return self._num_quantiles

    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """qrdqn.py:58-68: the target network's quantiles of the online network's greedy
        action at s_{t+n}, [bsz, N].  Only obs_next is gathered."""
        obs_next = buffer.get(indices, "obs_next") if getattr(buffer, "_save_obs_next", True) \
            else buffer[indices].obs_next
        return self._next_rows(Batch(obs_next=obs_next, info=Batch()))

    def compute_q_value(self, logits: torch.Tensor, mask) -> torch.Tensor:
        """qrdqn.py:70-73."""
        return super().compute_q_value(logits.mean(2), mask)

    def _fused_loss(self, q, act, returns, weight, aux, td_out, loss_out):
        return _QRLoss.apply(q, (act, returns, self.tau_hat.detach().reshape(-1), weight, td_out,
                                 loss_out))

    def _learn_torch(self, batch: Batch, weight):
        """The reference's op sequence as written (qrdqn.py:78-95); returns the loss and the
        priorities that leave as ``batch.weight``."""
        self.optim.zero_grad()
        curr_dist = self(batch).logits
        n = len(curr_dist)
        act = torch.as_tensor(batch.act, device=curr_dist.device).reshape(n).long()
        curr_dist = curr_dist[torch.arange(n, device=curr_dist.device), act, :].unsqueeze(2)
        target_dist = torch.as_tensor(batch.returns, device=curr_dist.device).unsqueeze(1)
        dist_diff = F.smooth_l1_loss(target_dist, curr_dist, reduction="none")
        huber_loss = (dist_diff * (self.tau_hat - (target_dist - curr_dist).detach().le(0.)
                                   .float()).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else torch.as_tensor(weight, device=curr_dist.device) \
            .to(curr_dist.dtype)
        loss = (huber_loss * w).mean()
        prio = dist_diff.detach().abs().sum(-1).mean(1)
        loss.backward()
        self.optim.step()
        return loss.detach(), prio
