"""DiscreteSACPolicy (tianshou/policy/modelfree/discrete_sac.py:11-161): soft actor-critic for
discrete actions (arXiv:1910.07207) -- a categorical actor, twin critics over all actions and
an optional automatically tuned temperature -- on SACPolicy's device path (policy/sac.py,
policy/ddpg.py).

The kernels of csrc/dsac.hip carry the glue around the three forwards: ``tsrl_dsac_target``
(the soft state value of ``_target_q``: softmax, entropy, the min over the critics and the
expectation in one launch), ``tsrl_dsac_q_loss_fwd_bwd`` (both critics' gathered TD errors,
losses and full [b, A] gradients) and ``tsrl_dsac_actor_loss_fwd_bwd`` (actor and temperature
losses with the analytic gradient towards the logits).  Flat storage, ``tsrl_soft_update``,
the temperature's one-parameter FlatAdam and the HIP-graph replay of one update are
SACPolicy's; an update has no random input at all.  The kernels take the actor's output as
logits whatever it is: raw scores (``softmax_output=False``) or, as with the reference's
default ``softmax_output=True``, probabilities fed in as logits.

Differences from the reference: on the fused path ``_target_q`` draws no sample (the
reference's forward samples an action there that nobody reads), so torch's generator is not
advanced by ``process_fn`` or ``learn``; ``dist`` is built with ``validate_args=False`` and a
train-mode action is ``gumbel_sample`` (policy/pg.py: the same distribution in one launch) in
place of ``dist.sample()``; ``batch.weight`` leaves as an f32 device tensor.  ``fused = False``
is the reference's op sequence, the comparison leg and the CPU path.

What stays on torch is what stays there for SACPolicy.  Not built: ``obs.mask`` support, and a
conv trunk shared between the actor and the critics under graph replay (each network here owns
its parameters).  An actor that masks illegal actions itself, with -inf logits, is safe on
either path: the kernels give such an entry probability 0 and gradient exactly 0, as torch's
Categorical does (tests/test_gpu_offpolicy_edges.py).
"""
from typing import Any, Optional, Tuple, Union

import numpy as np
import torch
from torch.distributions import Categorical

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.flat_learn import KernelGradLoss, _partials
from tianshou_amd.policy.pg import gumbel_sample
from tianshou_amd.policy.sac import SACPolicy


def _table(t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError(f"expected a [b, num_actions] table, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def dsac_target_device(logits: torch.Tensor, q1: torch.Tensor, q2: torch.Tensor,
                       alpha: torch.Tensor) -> torch.Tensor:
    """discrete_sac.py:93-97: sum_a p_a min(q1, q2)_a + alpha * entropy over [b, A] rows,
    alpha a one-element f32 device tensor; [b] f32."""
    l, a, c = _table(logits), _table(q1), _table(q2)
    if not l.shape == a.shape == c.shape or alpha.numel() != 1:
        raise ValueError("dsac_target_device: logits, q1 and q2 need one [b, A] shape, alpha "
                         "one element")
    b, A = l.shape
    out = torch.empty(b, dtype=torch.float32, device=l.device)
    _C.check(_C.lib().tsrl_dsac_target(_C.ptr(l), _C.ptr(a), _C.ptr(c),
                                       _C.ptr(alpha, torch.float32), b, A, _C.ptr(out),
                                       _C.stream_ptr(l.device)), "tsrl_dsac_target")
    return out


class _DsacQLoss(KernelGradLoss):
    """discrete_sac.py:108-124 for both critics as tsrl_dsac_q_loss_fwd_bwd.  The output is the
    sum of the two losses, the handle to call backward on; the per-critic losses and the
    per-row vector are written to ``loss`` / ``td`` (see dsac_q_loss)."""

    @staticmethod
    def forward(ctx, args, q1, q2):
        act, returns, weight, td, loss = args
        x = [_table(q1), _table(q2)]
        b, A = x[0].shape
        dev = x[0].device
        if x[1].shape != x[0].shape or loss.numel() != 2 or act.dtype != torch.int64 or not all(
                t is None or t.numel() == b for t in (act, returns, weight, td)):
            raise ValueError(f"_DsacQLoss: q1 and q2 need one [b, A] shape, act (int64), "
                             f"returns, weight and td {b} elements each, loss two")
        grads = [torch.empty_like(t) for t in x]
        total = torch.empty((), dtype=torch.float32, device=dev)
        _C.check(_C.lib().tsrl_dsac_q_loss_fwd_bwd(
            _C.ptr(x[0]), _C.ptr(x[1]), _C.ptr(act, torch.int64), _C.ptr(returns, torch.float32),
            _C.ptr(weight, torch.float32), b, A, _C.ptr(grads[0]), _C.ptr(grads[1]),
            _C.ptr(td, torch.float32), _C.ptr(_partials(b, 2, dev)),
            _C.ptr(loss, torch.float32), _C.ptr(total), _C.stream_ptr(dev)),
            "tsrl_dsac_q_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q1, q2))
        return total


def dsac_q_loss(q1: torch.Tensor, q2: torch.Tensor, act: torch.Tensor, returns: torch.Tensor,
                weight: Optional[torch.Tensor], td_out: Optional[torch.Tensor] = None,
                loss_out: Optional[torch.Tensor] = None):
    """(handle, losses [2], per-row vector [b]) of the critics' Q tables ([b, A] each) at the
    int64 actions ``act`` [b]: ``handle.backward()`` hands every critic the gradient of its
    own loss.  ``td_out`` / ``loss_out`` receive the outputs in place (the static outputs of a
    captured graph)."""
    dev, b = q1.device, q1.shape[0]
    td = torch.empty(b, dtype=torch.float32, device=dev) if td_out is None else td_out
    loss = torch.empty(2, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    return _DsacQLoss.apply((act, returns, weight, td, loss), q1, q2), loss, td


class _DsacActorLoss(KernelGradLoss):
    """discrete_sac.py:127-133 and 138-140 as tsrl_dsac_actor_loss_fwd_bwd.  The output is the
    handle to call backward on (towards the logits alone: the critics' tables are constants);
    the losses go to ``loss`` and the temperature's gradient to ``g_log_alpha``."""

    @staticmethod
    def forward(ctx, args, logits):
        q1, q2, alpha, log_alpha, target_entropy, loss, g_log_alpha = args
        l, a, c = _table(logits), _table(q1), _table(q2)
        b, A = l.shape
        dev = l.device
        if not l.shape == a.shape == c.shape or alpha.numel() != 1 or loss.numel() != (
                1 if log_alpha is None else 2):
            raise ValueError("_DsacActorLoss: logits, q1 and q2 need one [b, A] shape, alpha "
                             "one element, loss one (two with log_alpha)")
        grad = torch.empty_like(l)
        _C.check(_C.lib().tsrl_dsac_actor_loss_fwd_bwd(
            _C.ptr(l), _C.ptr(a), _C.ptr(c), _C.ptr(alpha, torch.float32),
            _C.ptr(log_alpha, torch.float32), float(target_entropy), b, A, _C.ptr(grad),
            _C.ptr(_partials(b, 2, dev)), _C.ptr(loss, torch.float32),
            _C.ptr(g_log_alpha, torch.float32), _C.stream_ptr(dev)),
            "tsrl_dsac_actor_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, (grad,), (logits,))
        return torch.empty((), dtype=torch.float32, device=dev)


def dsac_actor_loss(logits: torch.Tensor, q1: torch.Tensor, q2: torch.Tensor,
                    alpha: torch.Tensor, log_alpha: Optional[torch.Tensor] = None,
                    target_entropy: float = 0.0, loss_out: Optional[torch.Tensor] = None,
                    g_log_alpha_out: Optional[torch.Tensor] = None):
    """(handle, losses, g_log_alpha): ``handle.backward()`` hands the logits the gradient of the
    actor loss -mean(alpha * entropy + sum_a p_a min(q1, q2)_a) = losses[0].  With ``log_alpha``
    (one f32 element) losses[1] is the temperature loss and g_log_alpha its gradient.
    ``loss_out`` / ``g_log_alpha_out`` receive the outputs in place."""
    dev = logits.device
    auto = log_alpha is not None
    loss = torch.empty(2 if auto else 1, dtype=torch.float32, device=dev) if loss_out is None \
        else loss_out
    g_la = g_log_alpha_out
    if auto and g_la is None:
        g_la = torch.empty(1, dtype=torch.float32, device=dev)
    la = None if not auto else log_alpha.detach()
    handle = _DsacActorLoss.apply((q1, q2, alpha, la, target_entropy, loss, g_la), logits)
    return handle, loss, g_la


class DiscreteSACPolicy(SACPolicy):
    """Constructor arguments and defaults as the reference's (discrete_sac.py:40-70);
    ``deterministic_eval`` arrives through ``**kwargs``.  The device-path attributes are
    DDPGPolicy's."""

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critic1: torch.nn.Module, critic1_optim: torch.optim.Optimizer,
                 critic2: torch.nn.Module, critic2_optim: torch.optim.Optimizer,
                 tau: float = 0.005, gamma: float = 0.99,
                 alpha: Union[float, Tuple[float, torch.Tensor, torch.optim.Optimizer]] = 0.2,
                 reward_normalization: bool = False, estimation_step: int = 1,
                 **kwargs: Any) -> None:
        super().__init__(actor, actor_optim, critic1, critic1_optim, critic2, critic2_optim,
                         tau, gamma, alpha, reward_normalization, estimation_step,
                         action_scaling=False, action_bound_method=None, **kwargs)
        # the reference's value; BasePolicy's constructor (as the reference's) asserts against
        # the empty string, and map_action reads it as None: no bounding
        self.action_bound_method = ""

    # -- acting ---------------------------------------------------------------------------------
    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                input: str = "obs", **kwargs: Any) -> Batch:
        """discrete_sac.py:73-87.  Fused: a train-mode action is one gumbel_sample launch."""
        obs = batch[input]
        logits, hidden = self.actor(obs, state=state, info=batch.get("info", Batch()))
        fused = self.fused and logits.is_cuda
        dist = Categorical(logits=logits, validate_args=False) if fused else \
            Categorical(logits=logits)
        if self._deterministic_eval and not self.training:
            act = logits.argmax(dim=-1)
        elif fused and logits.dim() == 2 and logits.dtype == torch.float32:
            act = gumbel_sample(logits.detach())
        else:
            act = dist.sample()
        return Batch(logits=logits, act=act, state=hidden, dist=dist)

    def exploration_noise(self, act, batch: Batch):
        """discrete_sac.py:159-161."""
        return act

    # -- process_fn -----------------------------------------------------------------------------
    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """discrete_sac.py:89-98: the soft state value of the target critics under the
        actor's distribution.  Fused: the three forwards and one tsrl_dsac_target launch."""
        obs_next = self._obs_next(buffer, indices)
        if not (self.fused and self._on_device()):
            dist = self(Batch(obs_next=obs_next, info=Batch()), input="obs_next").dist
            target_q = dist.probs * torch.min(self.critic1_old(obs_next),
                                              self.critic2_old(obs_next))
            return target_q.sum(dim=-1) + self._alpha * dist.entropy()
        logits, _ = self.actor(obs_next, state=None, info=Batch())
        return dsac_target_device(logits, self.critic1_old(obs_next), self.critic2_old(obs_next),
                                  self._alpha_tensor(logits.device))

    # -- learn ----------------------------------------------------------------------------------
    def _learn_act(self, batch: Batch, dev, n: int) -> torch.Tensor:
        return torch.as_tensor(batch.act, device=dev).to(torch.int64).reshape(n).contiguous()

    def _learn_draws(self, act: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        return ()

    def _learn_torch(self, batch: Batch, do_actor: bool):
        """The reference's op sequence as written (discrete_sac.py:100-146)."""
        weight = batch.get("weight", None)
        dev = next(self.critic1.parameters()).device
        target_q = torch.as_tensor(batch.returns, device=dev).flatten()
        if weight is None:
            weight = 1.0
        elif not isinstance(weight, float):
            weight = torch.as_tensor(weight, device=dev).to(target_q.dtype)
        act = torch.as_tensor(batch.act, device=dev).to(torch.long).reshape(-1, 1)
        current_q1 = self.critic1(batch.obs).gather(1, act).flatten()
        td1 = current_q1 - target_q
        critic1_loss = (td1.pow(2) * weight).mean()
        self.critic1_optim.zero_grad()
        critic1_loss.backward()
        self.critic1_optim.step()
        current_q2 = self.critic2(batch.obs).gather(1, act).flatten()
        td2 = current_q2 - target_q
        critic2_loss = (td2.pow(2) * weight).mean()
        self.critic2_optim.zero_grad()
        critic2_loss.backward()
        self.critic2_optim.step()
        td = ((td1 + td2) / 2.0).detach()
        dist = self(batch).dist
        entropy = dist.entropy()
        with torch.no_grad():
            q = torch.min(self.critic1(batch.obs), self.critic2(batch.obs))
        actor_loss = -(self._alpha * entropy + (dist.probs * q).sum(dim=-1)).mean()
        self.actor_optim.zero_grad()
        actor_loss.backward()
        self.actor_optim.step()
        losses = [critic1_loss.detach(), critic2_loss.detach(), actor_loss.detach()]
        if self._is_auto_alpha:
            log_prob = -entropy.detach() + self._target_entropy
            alpha_loss = -(self._log_alpha * log_prob).mean()
            self._alpha_optim.zero_grad()
            alpha_loss.backward()
            self._alpha_optim.step()
            self._alpha = self._log_alpha.detach().exp()
            losses += [alpha_loss.detach(), self._alpha.reshape(())]
        self.sync_weight()
        return torch.stack([t.to(torch.float32) for t in losses]), td

    def _step(self, fas, obs, act, returns, weight, do_actor: bool, td_out: torch.Tensor,
              loss_out: torch.Tensor) -> None:
        """One update (discrete_sac.py:100-146): both critics' forward, their fused losses,
        backward and optimiser passes; the actor's forward, both stepped critics without
        gradient, the fused actor / temperature loss, backward into the actor and its optimiser
        pass; the temperature's optimiser pass and alpha = exp(log_alpha) in place; the soft
        update.  loss_out: critic1, critic2, actor (, temperature loss, alpha)."""
        names = self._critic_names
        handle, _, _ = dsac_q_loss(self.critic1(obs), self.critic2(obs), act, returns, weight,
                                   td_out, loss_out[:2])
        self._backward_step(handle, names, fas)
        logits, _ = self.actor(obs, state=None, info=Batch())
        with torch.no_grad():
            q1a, q2a = self.critic1(obs), self.critic2(obs)
        alpha = self._alpha_tensor(logits.device)
        if not self._is_auto_alpha:
            handle, _, _ = dsac_actor_loss(logits, q1a, q2a, alpha, loss_out=loss_out[2:3])
            self._backward_step(handle, ("actor",), fas)
            self.sync_weight()
            return
        fa = self._alpha_flat()
        handle, _, g_la = dsac_actor_loss(
            logits, q1a, q2a, alpha, self._log_alpha, self._target_entropy, loss_out[2:4],
            None if fa is None else fa.flat_grad)  # the gradient lands in log_alpha's .grad
        self._backward_step(handle, ("actor",), fas)
        if fa is not None:
            fa.clip_adam(None)
            torch.exp(self._log_alpha.detach(), out=alpha)
        else:  # another optimiser: torch's step on the kernel's gradient
            self._alpha_optim.zero_grad()
            self._log_alpha.grad = g_la.to(self._log_alpha.dtype).view_as(self._log_alpha)
            self._alpha_optim.step()
            alpha.copy_(self._log_alpha.detach().exp())
        loss_out[4:5].copy_(alpha)
        self.sync_weight()
