"""REDQPolicy (tianshou/policy/modelfree/redq.py:13-200): randomised ensembled double
Q-learning -- one critic ensemble network (utils/net.py ``EnsembleLinear`` layers, output
[E, b, 1]), a target built from a random subset of its target copy, a tanh-squashed Gaussian
actor stepped every ``actor_delay`` critic steps and an optional automatically tuned
temperature -- on DDPGPolicy's device path (policy/ddpg.py), with SACPolicy's sample kernels,
device-resident temperature and one-parameter FlatAdam (policy/sac.py).

REDQ's point is a high update-to-data ratio (20 updates per environment step in
examples/mujoco/mujoco_redq.py), so ``update()`` is the hot path.  The kernels of csrc/redq.hip
carry its glue: ``tsrl_redq_target`` (min / mean over the drawn subset less alpha * log_prob),
``tsrl_redq_q_loss_fwd_bwd`` (the ensemble's TD error, loss, gradient and per-row mean TD
error) and ``tsrl_redq_actor_loss_fwd_bwd`` (actor and temperature losses on the ensemble
mean, every gradient).  The sample is ``tsrl_sac_sample_fwd`` / ``_bwd`` through ``sac_sample``.
With plain Adam / RMSprop optimisers an update replays from one of two captured HIP graphs per
shape: the critics' step and the soft update, or those around the actor and temperature steps.
A critic-only update reads no random input.

The subset is drawn on the host by ``np.random.choice(ensemble_size, subset_size,
replace=False)`` after the actor's forward, where the reference draws it, and uploaded as int32.
The learn-time N(0, 1) draw is made only on updates that step the actor, so both random streams
stay the reference's.

Differences from the reference: those policy/sac.py lists (``validate_args=False`` on the fused
path, f32 device ``batch.weight`` and actions), and ``loss/actor`` is a float -- the reference
returns a 1-tuple because of a stray comma (redq.py:195).  ``fused = False`` is the reference's
op sequence, the comparison leg and the CPU path.

Not built: evaluating only the sampled subset of target critics, fusing the ensemble's H -> 1
head with the loss, a hand-written ensemble GEMM, data-parallel REDQ and a fused collect step.
"""
from copy import deepcopy
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.exploration import BaseNoise
from tianshou_amd.policy.ddpg import DDPGPolicy
from tianshou_amd.policy.flat_learn import KernelGradLoss, _partials
from tianshou_amd.policy.sac import _rows, _SquashedGaussianMixin, sac_sample

TARGET_MODES = {"min": 0, "mean": 1}


def redq_target_device(qs: torch.Tensor, idx: np.ndarray, mode: str, log_prob: torch.Tensor,
                       alpha: torch.Tensor) -> torch.Tensor:
    """redq.py:150-155: min or mean over the members ``idx`` (the host's draw) of ``qs``
    [E, b, 1] less alpha * log_prob, alpha a one-element f32 device tensor; the result is
    [b, 1].  An index outside [0, E) or a subset larger than the ensemble raises."""
    if qs.dim() < 2 or mode not in TARGET_MODES:
        raise ValueError(f"redq_target_device: qs {tuple(qs.shape)} needs [E, b(, 1)] and mode "
                         f"{mode!r} one of {tuple(TARGET_MODES)}")
    E = qs.shape[0]
    q, lp = _rows(qs).view(E, -1), _rows(log_prob).view(-1)
    b = q.shape[1]
    host = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int32)
    if lp.numel() != b or alpha.numel() != 1:
        raise ValueError("redq_target_device: log_prob needs one element per column of qs, "
                         "alpha one element")
    dev_idx = torch.as_tensor(host, device=q.device)
    out = torch.empty(b, dtype=torch.float32, device=q.device)
    _C.check(_C.lib().tsrl_redq_target(
        _C.ptr(q), E, b, _C.ptr(dev_idx, torch.int32), host.ctypes.data, host.size,
        TARGET_MODES[mode], _C.ptr(lp), _C.ptr(alpha, torch.float32), _C.ptr(out),
        _C.stream_ptr(q.device)), "tsrl_redq_target")
    return out.view(b, 1)


class _RedqQLoss(KernelGradLoss):
    """redq.py:161-169 as tsrl_redq_q_loss_fwd_bwd.  The output is the handle to call backward
    on; the loss and the per-row mean TD error go to ``loss`` / ``td`` (see redq_q_loss)."""

    @staticmethod
    def forward(ctx, args, q):
        returns, weight, td, loss = args
        if q.dim() != 2:
            raise ValueError(f"_RedqQLoss: q {tuple(q.shape)} needs [E, b]")
        x = _rows(q)
        (E, b), dev = x.shape, x.device
        if loss.numel() != 1 or not all(t is None or t.numel() == b
                                        for t in (returns, weight, td)):
            raise ValueError(f"_RedqQLoss: returns, weight and td need {b} elements each, loss "
                             "one")
        grad = torch.empty_like(x)
        _C.check(_C.lib().tsrl_redq_q_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(returns, torch.float32), _C.ptr(weight, torch.float32), E, b,
            _C.ptr(grad), _C.ptr(td, torch.float32), _C.ptr(_partials(b, 1, dev)),
            _C.ptr(loss, torch.float32), _C.stream_ptr(dev)), "tsrl_redq_q_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, (grad,), (q,))
        return torch.empty((), dtype=torch.float32, device=dev)


def redq_q_loss(q: torch.Tensor, returns: torch.Tensor, weight: Optional[torch.Tensor],
                td_out: Optional[torch.Tensor] = None, loss_out: Optional[torch.Tensor] = None):
    """(handle, loss [1], mean TD error [b]) of the ensemble's output ``q`` [E, b]:
    ``handle.backward()`` hands q the gradient of mean(weight * (q - returns)^2).  ``td_out`` /
    ``loss_out`` receive the outputs in place (the static outputs of a captured graph)."""
    dev, b = q.device, q.shape[-1]
    td = torch.empty(b, dtype=torch.float32, device=dev) if td_out is None else td_out
    loss = torch.empty(1, dtype=torch.float32, device=dev) if loss_out is None else loss_out
    return _RedqQLoss.apply((returns, weight, td, loss), q), loss, td


class _RedqActorLoss(KernelGradLoss):
    """redq.py:176-189 as tsrl_redq_actor_loss_fwd_bwd.  The output is the handle to call
    backward on (towards q and log_prob); the losses go to ``loss`` and the temperature's
    gradient to ``g_log_alpha`` (see redq_actor_loss)."""

    @staticmethod
    def forward(ctx, args, q, log_prob):
        alpha, log_alpha, target_entropy, loss, g_log_alpha = args
        if q.dim() != 2:
            raise ValueError(f"_RedqActorLoss: q {tuple(q.shape)} needs [E, b]")
        x, lp = _rows(q), _rows(log_prob).view(-1)
        (E, b), dev = x.shape, x.device
        if lp.numel() != b or alpha.numel() != 1 or loss.numel() != (
                1 if log_alpha is None else 2):
            raise ValueError(f"_RedqActorLoss: log_prob needs {b} elements, alpha one, loss one "
                             "(two with log_alpha)")
        gq, glp = torch.empty_like(x), torch.empty_like(lp)
        _C.check(_C.lib().tsrl_redq_actor_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(lp), _C.ptr(alpha, torch.float32),
            _C.ptr(log_alpha, torch.float32), float(target_entropy), E, b, _C.ptr(gq),
            _C.ptr(glp), _C.ptr(_partials(b, 2, dev)), _C.ptr(loss, torch.float32),
            _C.ptr(g_log_alpha, torch.float32), _C.stream_ptr(dev)),
            "tsrl_redq_actor_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, (gq, glp), (q, log_prob))
        return torch.empty((), dtype=torch.float32, device=dev)


def redq_actor_loss(q: torch.Tensor, log_prob: torch.Tensor, alpha: torch.Tensor,
                    log_alpha: Optional[torch.Tensor] = None, target_entropy: float = 0.0,
                    loss_out: Optional[torch.Tensor] = None,
                    g_log_alpha_out: Optional[torch.Tensor] = None):
    """(handle, losses, g_log_alpha): ``handle.backward()`` hands q [E, b] and log_prob [b] the
    gradient of the actor loss mean(alpha * log_prob - mean_e q) = losses[0].  With
    ``log_alpha`` (one f32 element) losses[1] is the temperature loss and g_log_alpha its
    gradient.  ``loss_out`` / ``g_log_alpha_out`` receive the outputs in place."""
    dev = q.device
    auto = log_alpha is not None
    loss = torch.empty(2 if auto else 1, dtype=torch.float32, device=dev) if loss_out is None \
        else loss_out
    g_la = g_log_alpha_out
    if auto and g_la is None:
        g_la = torch.empty(1, dtype=torch.float32, device=dev)
    la = None if not auto else log_alpha.detach()
    handle = _RedqActorLoss.apply((alpha, la, target_entropy, loss, g_la), q, log_prob)
    return handle, loss, g_la


class REDQPolicy(_SquashedGaussianMixin, DDPGPolicy):
    """Constructor arguments, defaults, assertions and the ValueError as the reference's
    (redq.py:55-105); the device-path attributes are DDPGPolicy's."""

    _critic_names = ("critics",)
    _sync_order = ("critics",)  # redq.py:113-115: the actor has no target copy
    _optim_order = ("critics", "actor")
    # the Collector keeps this policy on its eager device step: every forward draws
    eager_collect_step = True

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critics: torch.nn.Module, critics_optim: torch.optim.Optimizer,
                 ensemble_size: int = 10, subset_size: int = 2, tau: float = 0.005,
                 gamma: float = 0.99,
                 alpha: Union[float, Tuple[float, torch.Tensor, torch.optim.Optimizer]] = 0.2,
                 reward_normalization: bool = False, estimation_step: int = 1,
                 actor_delay: int = 20, exploration_noise: Optional[BaseNoise] = None,
                 deterministic_eval: bool = True, target_mode: str = "min",
                 **kwargs: Any) -> None:
        super().__init__(None, None, None, None, tau, gamma, exploration_noise,
                         reward_normalization, estimation_step, **kwargs)
        self.actor, self.actor_optim = actor, actor_optim
        self.critics, self.critics_old = critics, deepcopy(critics)
        self.critics_old.eval()
        self.critics_optim = critics_optim
        assert 0 < subset_size <= ensemble_size, \
            "Invalid choice of ensemble size or subset size."
        self.ensemble_size = ensemble_size
        self.subset_size = subset_size
        self._init_temperature(alpha, deterministic_eval)
        if target_mode in TARGET_MODES:
            self.target_mode = target_mode
        else:
            raise ValueError("Unsupported mode of Q target computing.")
        self.critic_gradient_step = 0
        self.actor_delay = actor_delay

    # -- process_fn -----------------------------------------------------------------------------
    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """redq.py:143-157: min or mean over a random subset of the target ensemble at the
        sampled next action, less alpha times its log-probability."""
        obs_next = self._obs_next(buffer, indices)
        res = self(Batch(obs_next=obs_next, info=Batch()), input="obs_next")
        idx = np.random.choice(self.ensemble_size, self.subset_size, replace=False)
        qs = self.critics_old(obs_next, res.act)
        if self.fused and qs.is_cuda:
            return redq_target_device(qs, idx, self.target_mode, res.log_prob,
                                      self._alpha_tensor(qs.device))
        qs = qs[idx, ...]
        if self.target_mode == "min":
            target_q, _ = torch.min(qs, dim=0)
        else:
            target_q = torch.mean(qs, dim=0)
        target_q -= self._alpha * res.log_prob
        return target_q

    # -- learn ----------------------------------------------------------------------------------
    def _actor_step_due(self) -> bool:
        """redq.py:170-173, asked before ``critic_gradient_step`` counts this update."""
        return (self.critic_gradient_step + 1) % self.actor_delay == 0

    def _loss_slots(self) -> int:
        return 4 if self._is_auto_alpha else 2  # critics, actor (, temperature loss, alpha)

    def _result(self, losses: List[float], did_actor: bool) -> Dict[str, float]:
        """redq.py:170 and 193-200."""
        self.critic_gradient_step += 1
        result = {"loss/critics": losses[0]}
        if did_actor:
            result["loss/actor"] = losses[1]
            if self._is_auto_alpha:
                result["loss/alpha"] = losses[2]
                result["alpha"] = losses[3]
        return result

    def _learn_draws(self, act: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """The N(0, 1) draw of the actor step, on the updates that take it."""
        return super()._learn_draws(act) if self._actor_step_due() else ()

    def _learn_torch(self, batch: Batch, do_actor: bool):
        """The reference's op sequence as written (redq.py:159-191)."""
        weight = batch.get("weight", None)
        current_qs = self.critics(batch.obs, batch.act).flatten(1)
        target_q = torch.as_tensor(batch.returns, device=current_qs.device).flatten()
        td = current_qs - target_q
        if weight is None:
            weight = 1.0
        elif not isinstance(weight, float):
            weight = torch.as_tensor(weight, device=td.device).to(td.dtype)
        critic_loss = (td.pow(2) * weight).mean()
        self.critics_optim.zero_grad()
        critic_loss.backward()
        self.critics_optim.step()
        losses = [critic_loss.detach()]
        if do_actor:
            obs_result = self(batch)
            current_qa = self.critics(batch.obs, obs_result.act).mean(dim=0).flatten()
            actor_loss = (self._alpha * obs_result.log_prob.flatten() - current_qa).mean()
            self.actor_optim.zero_grad()
            actor_loss.backward()
            self.actor_optim.step()
            losses.append(actor_loss.detach())
            if self._is_auto_alpha:
                log_prob = obs_result.log_prob.detach() + self._target_entropy
                alpha_loss = -(self._log_alpha * log_prob).mean()
                self._alpha_optim.zero_grad()
                alpha_loss.backward()
                self._alpha_optim.step()
                self._alpha = self._log_alpha.detach().exp()
                losses += [alpha_loss.detach(), self._alpha.reshape(())]
        self.sync_weight()
        return torch.stack([t.to(torch.float32) for t in losses]), \
            torch.mean(td, dim=0).detach()

    def _step(self, fas, obs, act, returns, weight, do_actor: bool, td_out: torch.Tensor,
              loss_out: torch.Tensor, eps: Optional[torch.Tensor] = None) -> None:
        """One update (redq.py:159-191): the ensemble's forward, its fused loss, backward and
        optimiser pass; on actor updates the actor's forward, the sample kernel, the ensemble
        at the sampled action, the fused actor / temperature loss, backward into the actor
        alone and its optimiser pass, then the temperature's optimiser pass and alpha =
        exp(log_alpha) in place; the soft update.  loss_out: critics, actor (, temperature
        loss, alpha)."""
        q = self.critics(obs, act).flatten(1)
        handle, _, _ = redq_q_loss(q, returns, weight, td_out, loss_out[:1])
        self._backward_step(handle, ("critics",), fas)
        if do_actor:
            (mu, sigma), _ = self.actor(obs, state=None, info=Batch())
            a, log_prob = sac_sample(mu, sigma, eps)
            qa = self.critics(obs, a).flatten(1)
            alpha = self._alpha_tensor(a.device)
            if not self._is_auto_alpha:
                handle, _, _ = redq_actor_loss(qa, log_prob, alpha, loss_out=loss_out[1:2])
                self._backward_step(handle, ("actor",), fas)
            else:
                fa = self._alpha_flat()
                handle, _, g_la = redq_actor_loss(
                    qa, log_prob, alpha, self._log_alpha, self._target_entropy, loss_out[1:3],
                    None if fa is None else fa.flat_grad)  # lands in log_alpha's .grad
                self._backward_step(handle, ("actor",), fas)
                self._alpha_step(g_la, alpha)
                loss_out[3:4].copy_(alpha)
        self.sync_weight()
