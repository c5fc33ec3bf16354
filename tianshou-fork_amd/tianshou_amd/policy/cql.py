"""CQLPolicy (tianshou/policy/imitation/cql.py:13-288): conservative Q-learning on SACPolicy's
device path (policy/sac.py), trained from a fixed buffer by OfflineTrainer (trainer/base.py).

The kernels of csrc/offline_cont.hip carry CQL's own glue: ``tsrl_cql_expand`` (every repeated
observation row and the random actions, one launch), ``tsrl_cql_target`` (the 1-step
entropy-regularised target from rew, done and obs_next) and ``tsrl_cql_loss_fwd_bwd`` (both
critics' MSE and logsumexp terms, the Lagrange multiplier's loss and every gradient).  The actor
and temperature step is SAC's (``tsrl_sac_sample_fwd`` / ``_bwd``,
``tsrl_sac_actor_loss_fwd_bwd``), the critics step through ``FlatAdam.clip_adam(clip_grad)``,
and with plain Adam / RMSprop optimisers an update replays from one captured HIP graph; its one
host read fetches the loss vector.

Each critic runs one forward over the stacked 3 b R rows (random, current-policy and next-policy
actions, all at the repeated ``obs``) and one over the b data rows, where the reference runs
four.  The actor runs one forward over 2 b R rows under ``no_grad``: the reference lets that
gradient reach the actor but zeroes it before the actor's next step, so the parameters evolve
identically.  Kept from the reference as written: its ``reshape`` calls in ``learn`` are no-ops,
so the logsumexp runs over the 3 columns of each of the b R rows; random actions come from
``uniform_(-min_action, max_action)``; ``process_fn`` returns the batch unchanged.

Every draw is made before the kernels run (a learn graph's static inputs): N(0, 1) through
``_rsample_noise``, U[0, 1) through ``_cql_uniform``, in the reference's order.

Difference from the reference: ``cql_log_alpha`` is a leaf on ``device`` and steps through a
one-parameter FlatAdam, exactly as SAC's ``log_alpha`` does.  At ``device="cpu"`` that is the
reference; on a GPU the reference's optimiser steps a host copy that its ``learn`` never reads,
so its multiplier stays at its initial value there.  ``fused = False`` is the reference's op
sequence (with the multiplier as above), the comparison leg and the CPU path.
Not built: data-parallel updates, u8 observations on the expand kernel.
"""
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn.utils import clip_grad_norm_

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import (KernelGradLoss, _partials, f32_rows,
                                            replay_learn_graph)
from tianshou_amd.policy.sac import SACPolicy, _rows, sac_actor_loss, sac_sample


def cql_expand(obs: torch.Tensor, obs_next: torch.Tensor, u: torch.Tensor, lo: float, hi: float,
               repeat: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(actor_in [2 n, ...], critic_obs [3 n, ...], critic_act [3 n, A]) with n = b * repeat, as
    one tsrl_cql_expand launch: row i * repeat + j repeats row i; actor_in is the repeated
    ``obs`` then the repeated ``obs_next``, critic_obs the repeated ``obs`` three times, and the
    first n rows of critic_act are lo + u * (hi - lo); the others are left for the sampled
    actions.  ``obs`` / ``obs_next``: contiguous f32 of one shape; ``u`` [n, A] f32."""
    b = obs.shape[0]
    n, tail = b * repeat, tuple(obs.shape[1:])
    D = int(np.prod(tail)) if tail else 1
    if obs_next.shape != obs.shape or u.dim() != 2 or u.shape[0] != n:
        raise ValueError(f"cql_expand: obs {tuple(obs.shape)}, obs_next {tuple(obs_next.shape)} "
                         f"and u {tuple(u.shape)} do not fit repeat {repeat}")
    A, dev = u.shape[1], obs.device
    actor_in = torch.empty((2 * n,) + tail, dtype=torch.float32, device=dev)
    critic_obs = torch.empty((3 * n,) + tail, dtype=torch.float32, device=dev)
    critic_act = torch.empty((3 * n, A), dtype=torch.float32, device=dev)
    _C.check(_C.lib().tsrl_cql_expand(
        _C.ptr(obs, torch.float32), _C.ptr(obs_next, torch.float32), _C.ptr(u, torch.float32),
        float(lo), float(hi), b, repeat, D, A, _C.ptr(actor_in), _C.ptr(critic_obs),
        _C.ptr(critic_act), _C.stream_ptr(dev)), "tsrl_cql_expand")
    return actor_in, critic_obs, critic_act


def cql_target_device(q1: torch.Tensor, q2: torch.Tensor, log_prob: torch.Tensor,
                      alpha: torch.Tensor, rew: torch.Tensor, done: torch.Tensor, gamma: float
                      ) -> torch.Tensor:
    """cql.py:185-194 as one tsrl_cql_target launch: rew + gamma * (1 - done) * (min(q1, q2) -
    alpha * log_prob) over [b] f32 rows, alpha a one-element f32 device tensor."""
    xs = [_rows(t).view(-1) for t in (q1, q2, log_prob, rew, done)]
    b = xs[0].numel()
    if not all(t.numel() == b for t in xs) or alpha.numel() != 1:
        raise ValueError(f"cql_target_device: q1, q2, log_prob, rew and done need {b} elements "
                         "each, alpha one")
    out = torch.empty_like(xs[0])
    _C.check(_C.lib().tsrl_cql_target(
        _C.ptr(xs[0]), _C.ptr(xs[1]), _C.ptr(xs[2]), _C.ptr(alpha, torch.float32), _C.ptr(xs[3]),
        _C.ptr(xs[4]), float(gamma), b, _C.ptr(out), _C.stream_ptr(out.device)),
        "tsrl_cql_target")
    return out


class _CQLLoss(KernelGradLoss):
    """cql.py:198-260 as tsrl_cql_loss_fwd_bwd.  args: (target [b], log_pi [2, n], cql_log_alpha
    or None, the policy's scalars, act_dim, loss [2], lagrange [2] or None, g_cql_log_alpha [1]
    or None).  The output is the handle to call backward on: towards q1, q2 [b] and v1, v2
    [3 n], each critic receiving the gradient of its own loss."""

    @staticmethod
    def forward(ctx, args, q1, q2, v1, v2):
        target, log_pi, log_alpha, scal, act_dim, loss, lagrange, g_la = args
        temperature, weight, threshold, amin, amax = scal
        xs = [_rows(t).view(-1) for t in (q1, q2, v1, v2)]
        b, dev = xs[0].numel(), xs[0].device
        n, rem = divmod(xs[2].numel(), 3)
        if rem or n % b or xs[1].numel() != b or xs[3].numel() != 3 * n or \
                target.numel() != b or log_pi.numel() != 2 * n or loss.numel() != 2:
            raise ValueError(f"_CQLLoss: q1, q2 and target need {b} elements, v1 and v2 3 n and "
                             "log_pi 2 n with n a multiple of b, loss two")
        lag = log_alpha is not None
        if lag and (log_alpha.numel() != 1 or lagrange.numel() != 2 or g_la.numel() != 1):
            raise ValueError("_CQLLoss: the multiplier needs cql_log_alpha [1], lagrange [2] "
                             "and g_cql_log_alpha [1]")
        grads = [torch.empty_like(t) for t in xs]
        _C.check(_C.lib().tsrl_cql_loss_fwd_bwd(
            _C.ptr(xs[0]), _C.ptr(xs[1]), _C.ptr(target, torch.float32), _C.ptr(xs[2]),
            _C.ptr(xs[3]), _C.ptr(log_pi, torch.float32),
            _C.ptr(log_alpha, torch.float32) if lag else None, float(temperature), float(weight),
            float(threshold), float(amin), float(amax), int(act_dim), int(lag), b, n // b,
            *(_C.ptr(t) for t in grads), _C.ptr(_partials(n, 6, dev)),
            _C.ptr(loss, torch.float32), _C.ptr(lagrange, torch.float32) if lag else None,
            _C.ptr(g_la, torch.float32) if lag else None, _C.stream_ptr(dev)),
            "tsrl_cql_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q1, q2, v1, v2))
        return torch.empty((), dtype=torch.float32, device=dev)


class CQLPolicy(SACPolicy):
    """Constructor arguments, defaults and assertions as the reference's (cql.py:58-106); the
    device-path attributes are DDPGPolicy's."""

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critic1: torch.nn.Module, critic1_optim: torch.optim.Optimizer,
                 critic2: torch.nn.Module, critic2_optim: torch.optim.Optimizer,
                 cql_alpha_lr: float = 1e-4, cql_weight: float = 1.0, tau: float = 0.005,
                 gamma: float = 0.99,
                 alpha: Union[float, Tuple[float, torch.Tensor, torch.optim.Optimizer]] = 0.2,
                 temperature: float = 1.0, with_lagrange: bool = True,
                 lagrange_threshold: float = 10.0, min_action: float = -1.0,
                 max_action: float = 1.0, num_repeat_actions: int = 10, alpha_min: float = 0.0,
                 alpha_max: float = 1e6, clip_grad: float = 1.0,
                 device: Union[str, torch.device] = "cpu", **kwargs: Any) -> None:
        super().__init__(actor, actor_optim, critic1, critic1_optim, critic2, critic2_optim, tau,
                         gamma, alpha, **kwargs)
        self.device = device
        self.temperature = temperature
        self.with_lagrange = with_lagrange
        self.lagrange_threshold = lagrange_threshold
        self.cql_weight = cql_weight
        # a leaf on ``device`` (see the module docstring); not a Parameter, as in the reference
        self.cql_log_alpha = torch.zeros(1, dtype=torch.float32, device=device,
                                         requires_grad=True)
        self.cql_alpha_optim = torch.optim.Adam([self.cql_log_alpha], lr=cql_alpha_lr)
        self.min_action = min_action
        self.max_action = max_action
        self.num_repeat_actions = num_repeat_actions
        self.alpha_min = alpha_min
        self.alpha_max = alpha_max
        self.clip_grad = clip_grad
        self._cql_fa: Optional[FlatAdam] = None

    def process_fn(self, batch: Batch, buffer, indices: np.ndarray) -> Batch:
        """cql.py:157-160."""
        return batch

    def _cql_uniform(self, shape, device) -> torch.Tensor:
        """The U[0, 1) draw behind the random actions (cql.py:206-208); every path draws
        through here and scales it to [-min_action, max_action)."""
        return torch.rand(size=tuple(shape), device=device)

    # -- the reference's op sequence -------------------------------------------------------------
    def actor_pred(self, obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        res = self(Batch(obs=obs, info=Batch()))
        return res.act, res.log_prob

    def calc_pi_values(self, obs_pi: torch.Tensor, obs_to_pred: torch.Tensor
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
        act_pred, log_pi = self.actor_pred(obs_pi)
        q1, q2 = self.critic1(obs_to_pred, act_pred), self.critic2(obs_to_pred, act_pred)
        return q1 - log_pi.detach(), q2 - log_pi.detach()

    def _learn_reference(self, batch: Batch) -> torch.Tensor:
        """cql.py:162-288 as written, on the device the networks live on; returns the losses in
        the fused path's order (_result)."""
        dev = next(self.actor.parameters()).device

        def f32(x):
            return torch.as_tensor(x, device=dev).to(torch.float32)
        obs, act, rew, obs_next = f32(batch.obs), f32(batch.act), f32(batch.rew), \
            f32(batch.obs_next)
        done = f32(batch.done)
        batch_size, R, T, w = obs.shape[0], self.num_repeat_actions, self.temperature, \
            self.cql_weight
        act_pred, log_pi = self.actor_pred(obs)
        min_q = torch.min(self.critic1(obs, act_pred), self.critic2(obs, act_pred))
        actor_loss = (self._alpha * log_pi - min_q).mean()
        self.actor_optim.zero_grad()
        actor_loss.backward()
        self.actor_optim.step()
        losses = [actor_loss.detach()]
        if self._is_auto_alpha:
            log_pi = log_pi + self._target_entropy
            alpha_loss = -(self._log_alpha * log_pi.detach()).mean()
            self._alpha_optim.zero_grad()
            alpha_loss.backward()
            self._alpha_optim.step()
            self._alpha = self._log_alpha.detach().exp()
            losses += [alpha_loss.detach(), self._alpha.reshape(())]
        with torch.no_grad():
            act_next, new_log_pi = self.actor_pred(obs_next)
            target_q = torch.min(self.critic1_old(obs_next, act_next),
                                 self.critic2_old(obs_next, act_next)) - self._alpha * new_log_pi
            target_q = rew + self._gamma * (1 - done) * target_q.flatten()
        current_q1 = self.critic1(obs, act).flatten()
        current_q2 = self.critic2(obs, act).flatten()
        critic1_loss = F.mse_loss(current_q1, target_q)
        critic2_loss = F.mse_loss(current_q2, target_q)
        u = self._cql_uniform((batch_size * R, act.shape[-1]), dev).to(torch.float32)
        lo = -self.min_action
        random_actions = lo + u * (self.max_action - lo)
        repeat_size = [1, R] + [1] * (obs.dim() - 1)
        view_size = [batch_size * R] + list(obs.shape[1:])
        tmp_obs = obs.unsqueeze(1).repeat(*repeat_size).view(*view_size)
        tmp_obs_next = obs_next.unsqueeze(1).repeat(*repeat_size).view(*view_size)
        current_pi_value1, current_pi_value2 = self.calc_pi_values(tmp_obs, tmp_obs)
        next_pi_value1, next_pi_value2 = self.calc_pi_values(tmp_obs_next, tmp_obs)
        random_log_prob = np.log(0.5 ** random_actions.shape[-1])
        random_value1 = self.critic1(tmp_obs, random_actions) - random_log_prob
        random_value2 = self.critic2(tmp_obs, random_actions) - random_log_prob
        cat_q1 = torch.cat([random_value1, current_pi_value1, next_pi_value1], 1)
        cat_q2 = torch.cat([random_value2, current_pi_value2, next_pi_value2], 1)
        cql1 = torch.logsumexp(cat_q1 / T, dim=1).mean() * w * T - current_q1.mean() * w
        cql2 = torch.logsumexp(cat_q2 / T, dim=1).mean() * w * T - current_q2.mean() * w
        if self.with_lagrange:
            cql_alpha = torch.clamp(self.cql_log_alpha.exp(), self.alpha_min, self.alpha_max)
            cql1 = cql_alpha * (cql1 - self.lagrange_threshold)
            cql2 = cql_alpha * (cql2 - self.lagrange_threshold)
            self.cql_alpha_optim.zero_grad()
            cql_alpha_loss = -(cql1 + cql2) * 0.5
            cql_alpha_loss.backward(retain_graph=True)
            self.cql_alpha_optim.step()
            losses += [cql_alpha_loss.detach().reshape(()), cql_alpha.detach().reshape(())]
        critic1_loss = critic1_loss + cql1
        critic2_loss = critic2_loss + cql2
        self.critic1_optim.zero_grad()
        critic1_loss.backward(retain_graph=True)
        clip_grad_norm_(self.critic1.parameters(), self.clip_grad)
        self.critic1_optim.step()
        self.critic2_optim.zero_grad()
        critic2_loss.backward()
        clip_grad_norm_(self.critic2.parameters(), self.clip_grad)
        self.critic2_optim.step()
        self.sync_weight()
        losses = [critic1_loss.detach().reshape(()), critic2_loss.detach().reshape(())] + losses
        return torch.stack([t.to(torch.float32) for t in losses])

    # -- learn ----------------------------------------------------------------------------------
    def _loss_slots(self) -> int:
        return super()._loss_slots() + (2 if self.with_lagrange else 0)

    def _result(self, losses: List[float], did_actor: bool = True) -> Dict[str, float]:
        """cql.py:277-288."""
        result = super()._result(losses, did_actor)
        if self.with_lagrange:
            result["loss/cql_alpha"], result["cql_alpha"] = losses[-2], losses[-1]
        return result

    def _bind_cql_alpha(self) -> Optional[FlatAdam]:
        """The one-parameter flat storage of ``cql_log_alpha`` while ``cql_alpha_optim`` is a
        plain Adam / RMSprop over it (None: torch's step, and no graph)."""
        la = self.cql_log_alpha
        if not (self.with_lagrange and self.fused and self.fused_adam and la.is_cuda
                and la.dtype == torch.float32):
            return None
        if self._cql_fa is None:
            self._cql_fa = FlatAdam([la])
        fa = self._cql_fa
        if not fa.bind_adam(self.cql_alpha_optim):
            return None
        fa.bind_grads()
        fa.set_lr()
        return fa

    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        """cql.py:162-288; all losses come back in the update's one host read."""
        if not (self.fused and self._on_device()):
            return self._result(self._learn_reference(batch).tolist())
        self._bind_alpha()
        cql_fa = self._bind_cql_alpha()
        fas = {name: self._bind(name) for name in self._optim_order}
        dev = next(self.actor.parameters()).device
        n = len(batch.rew)
        obs = torch.as_tensor(batch.obs, device=dev)
        obs_next = torch.as_tensor(batch.obs_next, device=dev)
        act = self._learn_act(batch, dev, n)
        rew, done = f32_rows(batch.rew, dev, n), f32_rows(batch.done, dev, n)
        R, A = self.num_repeat_actions, act.shape[1]
        draws: Tuple[torch.Tensor, ...] = (
            *self._learn_draws(act), *self._learn_draws(act),
            _rows(self._cql_uniform((n * R, A), dev)))
        if self._draws():  # the current-policy rows, then the next-policy rows
            draws += (torch.cat([_rows(self._rsample_noise((n * R, A), dev)),
                                 _rows(self._rsample_noise((n * R, A), dev))]),)
        inputs = (obs, obs_next, act, rew, done, *draws)
        loss = None
        if all(fa is not None for fa in fas.values()):
            for fa in fas.values():
                fa.set_lr()
            if self._warm and self._graph_ok(obs, n) and self._expandable(obs, obs_next) and \
                    (cql_fa is not None or not self.with_lagrange):
                loss = self._graph_cql(fas, inputs)
        if loss is None:
            loss = torch.empty(self._loss_slots(), dtype=torch.float32, device=dev)
            self._cql_step(fas, inputs, loss)
        self._warm = True
        return self._result(loss.tolist())

    @staticmethod
    def _expandable(obs: torch.Tensor, obs_next: torch.Tensor) -> bool:
        return all(t.dtype == torch.float32 and t.is_contiguous() and t.dim() >= 2
                   for t in (obs, obs_next)) and obs.shape == obs_next.shape

    def _cql_flat(self) -> Optional[FlatAdam]:
        fa = self._cql_fa
        return fa if fa is not None and self.with_lagrange and \
            fa.adam_bound(self.cql_alpha_optim) else None

    def _cql_step(self, fas, inputs, loss_out: torch.Tensor) -> None:
        """One update in the reference's order: the actor and temperature step (SAC's kernels),
        the target, both critics at the data rows and at the stacked 3 b R rows, the fused CQL
        loss, the multiplier's step, the clipped critic steps, the soft update.  loss_out:
        critic1, critic2, actor (, temperature loss, alpha) (, multiplier loss, cql_alpha)."""
        obs, obs_next, act, rew, done, *draws = inputs
        draws = list(draws)
        sampling = self._draws()
        eps0, eps1 = (draws.pop(0), draws.pop(0)) if sampling else (None, None)
        u = draws.pop(0)
        eps2 = draws.pop(0) if sampling else None
        b, R, dev = len(rew), self.num_repeat_actions, rew.device
        n = b * R
        alpha = self._alpha_tensor(dev)
        # cql.py:168-182: the actor step, then the temperature's
        (mu, sigma), _ = self.actor(obs, state=None, info=Batch())
        a, log_prob = sac_sample(mu, sigma, eps0)
        q1a, q2a = self.critic1(obs, a).flatten(), self.critic2(obs, a).flatten()
        k = 3
        if not self._is_auto_alpha:
            handle, _, _ = sac_actor_loss(q1a, q2a, log_prob, alpha, loss_out=loss_out[2:3])
            self._backward_step(handle, ("actor",), fas)
        else:
            fa = self._alpha_flat()
            handle, _, g_la = sac_actor_loss(
                q1a, q2a, log_prob, alpha, self._log_alpha, self._target_entropy, loss_out[2:4],
                None if fa is None else fa.flat_grad)
            self._backward_step(handle, ("actor",), fas)
            self._alpha_step(g_la, alpha)
            loss_out[4:5].copy_(alpha)
            k = 5
        with torch.no_grad():
            # cql.py:185-194
            (mu, sigma), _ = self.actor(obs_next, state=None, info=Batch())
            a_next, lp_next = sac_sample(mu, sigma, eps1)
            target = cql_target_device(self.critic1_old(obs_next, a_next),
                                       self.critic2_old(obs_next, a_next), lp_next, alpha, rew,
                                       done, self._gamma)
            # cql.py:206-220: the repeated rows, the random and the sampled actions
            lo, hi = -self.min_action, self.max_action
            if self._expandable(obs, obs_next):
                actor_in, critic_obs, critic_act = cql_expand(obs, obs_next, u, lo, hi, R)
            else:
                rep = [1, R] + [1] * (obs.dim() - 1)
                shape = [n] + list(obs.shape[1:])
                tmp = obs.unsqueeze(1).repeat(*rep).view(*shape)
                actor_in = torch.cat([tmp, obs_next.unsqueeze(1).repeat(*rep).view(*shape)])
                critic_obs = torch.cat([tmp, tmp, tmp])
                critic_act = torch.empty((3 * n, u.shape[1]), dtype=torch.float32, device=dev)
                critic_act[:n] = lo + u * (hi - lo)
            (mu, sigma), _ = self.actor(actor_in, state=None, info=Batch())
            mu, sigma = _rows(mu), _rows(sigma)
            log_pi = torch.empty(2 * n, dtype=torch.float32, device=dev)
            _C.check(_C.lib().tsrl_sac_sample_fwd(
                _C.ptr(mu), _C.ptr(sigma), _C.ptr(eps2), 2 * n, mu.shape[1],
                _C.ptr(critic_act[n:]), _C.ptr(log_pi), _C.stream_ptr(dev)),
                "tsrl_sac_sample_fwd")
        # cql.py:198-260
        q1, q2 = self.critic1(obs, act).flatten(), self.critic2(obs, act).flatten()
        v1 = self.critic1(critic_obs, critic_act).flatten()
        v2 = self.critic2(critic_obs, critic_act).flatten()
        lag = self.with_lagrange
        cql_fa = self._cql_flat()
        g_la = None
        if lag:
            g_la = cql_fa.flat_grad if cql_fa is not None else \
                torch.empty(1, dtype=torch.float32, device=dev)
        handle = _CQLLoss.apply(
            (target, log_pi, self.cql_log_alpha.detach() if lag else None,
             (self.temperature, self.cql_weight, self.lagrange_threshold, self.alpha_min,
              self.alpha_max), critic_act.shape[1], loss_out[:2],
             loss_out[k:k + 2] if lag else None, g_la), q1, q2, v1, v2)
        if lag:  # cql.py:254-257
            if cql_fa is not None:  # the gradient landed in the multiplier's flat .grad
                cql_fa.clip_adam(None)
            else:
                self.cql_alpha_optim.zero_grad()
                self.cql_log_alpha.grad = g_la.to(self.cql_log_alpha.dtype)
                self.cql_alpha_optim.step()
        self._backward_step(handle, self._critic_names, fas, max_norm=self.clip_grad)
        self.sync_weight()

    def _graph_addr(self, fas) -> tuple:
        addr = super()._graph_addr(fas)
        if self._cql_flat() is None:
            return addr
        return addr + ((self.cql_log_alpha.data_ptr(), self._cql_fa.flat_grad.data_ptr()),)

    def _graph_cql(self, fas, inputs) -> Optional[torch.Tensor]:
        """One update replayed from a HIP graph captured once per (input shapes, observation
        dtype, flat addresses); None if the capture failed (this and every later update then
        run eagerly)."""
        dev = inputs[3].device
        key = tuple((tuple(t.shape), t.dtype) for t in inputs)
        out = replay_learn_graph(
            self._learn_graphs, key, self._graph_addr(fas), inputs,
            lambda: (torch.empty(1, dtype=torch.float32, device=dev),
                     torch.zeros(self._loss_slots(), dtype=torch.float32, device=dev)),
            lambda s, td, loss: self._cql_step(fas, s, loss), self._capture)
        if out is None:
            self._graph_failed = True
            return None
        return out[0]
