"""DiscreteCQLPolicy (tianshou/policy/imitation/discrete_cql.py:11-84): discrete conservative
Q-learning, arXiv:2006.04779, on QRDQNPolicy's device path.

Acting, ``_target_q``, the flat optimiser storage, the target mirror and the graph replay are
QRDQNPolicy's.  learn() is ``tsrl_cql_qr_loss_fwd_bwd`` (csrc/offline.hip): QR-DQN's pairwise
quantile Huber loss and priorities, the quantile means, their logsumexp and the dense
[b, A, N] gradient of ``qr + min_q_weight * cql`` in one launch, the three scalars in one device
vector.  ``batch.weight`` leaves as the QR priorities, as in the reference.  ``fused = False``
runs the reference's op sequence on torch, and so does learn() with more quantiles or actions
than the kernel stages (``_C.DIST_MAX_N``, ``_C.CQL_MAX_ACTIONS``).
"""
from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.offline import CQLLoss, backward_step
from tianshou_amd.policy.qrdqn import QRDQNPolicy


class DiscreteCQLPolicy(QRDQNPolicy):
    """Constructor arguments and defaults as the reference's (discrete_cql.py:34-50)."""

    def __init__(self, model: torch.nn.Module, optim: torch.optim.Optimizer,
                 discount_factor: float = 0.99, num_quantiles: int = 200,
                 estimation_step: int = 1, target_update_freq: int = 0,
                 reward_normalization: bool = False, min_q_weight: float = 10.0,
                 **kwargs: Any) -> None:
        super().__init__(model, optim, discount_factor, num_quantiles, estimation_step,
                         target_update_freq, reward_normalization, **kwargs)
        self._min_q_weight = min_q_weight

    def _fused_learn(self) -> bool:
        return super()._fused_learn() and \
            getattr(self, "max_action_num", 0) <= _C.CQL_MAX_ACTIONS

    def _loss_out(self, dev) -> torch.Tensor:
        """(loss, loss/qr, loss/cql)."""
        return torch.empty(3, dtype=torch.float32, device=dev)

    def _learn_result(self, loss: torch.Tensor) -> Dict[str, float]:
        total, qr_loss, min_q_loss = loss.tolist()
        return {"loss": total, "loss/qr": qr_loss, "loss/cql": min_q_loss}

    def _learn_torch(self, batch: Batch, weight):
        """The reference's op sequence as written (discrete_cql.py:55-78); returns the three
        scalars and the priorities that leave as ``batch.weight``."""
        self.optim.zero_grad()
        all_dist = self(batch).logits
        n = len(all_dist)
        act = torch.as_tensor(batch.act, device=all_dist.device).reshape(n).long()
        curr_dist = all_dist[torch.arange(n, device=all_dist.device), act, :].unsqueeze(2)
        target_dist = torch.as_tensor(batch.returns, device=all_dist.device).unsqueeze(1)
        dist_diff = F.smooth_l1_loss(target_dist, curr_dist, reduction="none")
        huber_loss = (dist_diff * (self.tau_hat - (target_dist - curr_dist).detach().le(0.)
                                   .float()).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else torch.as_tensor(weight, device=all_dist.device) \
            .to(all_dist.dtype)
        qr_loss = (huber_loss * w).mean()
        prio = dist_diff.detach().abs().sum(-1).mean(1)
        q = self.compute_q_value(all_dist, None)
        dataset_expec = q.gather(1, act.unsqueeze(1)).mean()
        negative_sampling = q.logsumexp(1).mean()
        min_q_loss = negative_sampling - dataset_expec
        loss = qr_loss + min_q_loss * self._min_q_weight
        loss.backward()
        self.optim.step()
        return torch.stack([loss, qr_loss, min_q_loss]).detach(), prio

    def _step(self, fa: Optional[FlatAdam], obs, info, act, returns, weight, *extra,
              td_out=None, loss_out=None):
        """Forward, the fused loss, backward, one optimiser step; returns (the three scalars
        as a device vector, the priorities)."""
        dist = self.model(obs, state=None, info=info)[0]
        out = self._loss_out(dist.device) if loss_out is None else loss_out
        prio = torch.empty(len(act), dtype=torch.float32, device=dist.device) \
            if td_out is None else td_out
        handle = CQLLoss.apply((act, returns, self.tau_hat.detach().reshape(-1), weight,
                                self._min_q_weight, prio, out), dist)
        backward_step(handle, fa, self.optim)
        return out, prio
