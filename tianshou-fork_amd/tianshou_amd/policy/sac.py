"""SACPolicy (tianshou/policy/modelfree/sac.py:13-190): soft actor-critic with twin critics, a
tanh-squashed Gaussian actor and an optional automatically tuned temperature, on DDPGPolicy's
device path (policy/ddpg.py).

The kernels of csrc/sac.hip carry SAC's own glue: ``tsrl_sac_sample_fwd`` / ``_bwd`` (the
reparameterised sample, its squashing and corrected log-probability, and the analytic
gradient, behind one autograd Function), ``tsrl_sac_target`` (the entropy-regularised target)
and ``tsrl_sac_actor_loss_fwd_bwd`` (actor and temperature losses with every gradient).  The
critics' losses are TD3's ``tsrl_q_mse_fwd_bwd`` launch, ``sync_weight`` one
``tsrl_soft_update`` launch over both critics, and with plain Adam / RMSprop optimisers an
update replays from one captured HIP graph per shape.  The temperature lives in a persistent
one-element device tensor that every kernel reads, so the automatic step moves it inside the
graph; ``log_alpha`` steps through a one-parameter FlatAdam.

Every N(0, 1) draw comes from ``_rsample_noise`` (``torch.randn`` on the device), made before
the kernels run: a learn graph holds no random generator, its draw is a static input.

Differences from the reference: on the fused path ``dist`` is built with
``validate_args=False`` (no launch and no host sync for the argument check; the torch leg
validates as the reference does), and ``batch.weight`` and the actions are f32 device tensors.
``fused = False`` is the reference's op sequence, the comparison leg and the CPU path.

DiscreteSACPolicy (policy/discrete_sac.py) subclasses this class; REDQPolicy (policy/redq.py)
shares _SquashedGaussianMixin with it; OffpolicyTrainer (trainer/base.py) drives all three.
Not built: data-parallel updates.
"""
from copy import deepcopy
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
from torch.distributions import Independent, Normal

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.exploration import BaseNoise
from tianshou_amd.policy.ddpg import DDPGPolicy, q_mse_loss
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import KernelGradLoss, _partials

EPS32 = np.finfo(np.float32).eps.item()


def _rows(t: torch.Tensor, shape=None) -> torch.Tensor:
    t = t.detach().to(torch.float32)
    return (t if shape is None else t.expand(shape)).contiguous()


class _SacSample(torch.autograd.Function):
    """sac.py:117-128 as tsrl_sac_sample_fwd: (act [b, A], log_prob [b]) of mu, sigma and the
    draw eps (None: the deterministic action tanh(mu)); backward is tsrl_sac_sample_bwd."""

    @staticmethod
    def forward(ctx, eps, mu, sigma):
        if mu.dim() != 2 or sigma.shape != mu.shape or (eps is not None
                                                        and eps.shape != mu.shape):
            raise ValueError(f"_SacSample: mu {tuple(mu.shape)}, sigma {tuple(sigma.shape)} "
                             "and eps need one [b, A] shape")
        m, s = _rows(mu), _rows(sigma)
        e = None if eps is None else _rows(eps)
        b, A = m.shape
        act = torch.empty_like(m)
        log_prob = torch.empty(b, dtype=torch.float32, device=m.device)
        _C.check(_C.lib().tsrl_sac_sample_fwd(_C.ptr(m), _C.ptr(s), _C.ptr(e), b, A,
                                              _C.ptr(act), _C.ptr(log_prob),
                                              _C.stream_ptr(m.device)), "tsrl_sac_sample_fwd")
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None
        ctx.save_for_backward(s, act, *(() if e is None else (e,)))
        ctx.meta = (mu.dtype, sigma.dtype)
        return act, log_prob

    @staticmethod
    def backward(ctx, g_act, g_logp):
        s, act, *rest = ctx.saved_tensors
        e = rest[0] if rest else None
        b, A = act.shape
        ga = None if g_act is None else _rows(g_act, act.shape)
        gl = None if g_logp is None else _rows(g_logp, (b,))
        if ga is None and gl is None:
            return None, None, None
        g_mu, g_sigma = torch.empty_like(act), torch.empty_like(act)
        _C.check(_C.lib().tsrl_sac_sample_bwd(_C.ptr(s), _C.ptr(e), _C.ptr(act), _C.ptr(ga),
                                              _C.ptr(gl), b, A, _C.ptr(g_mu), _C.ptr(g_sigma),
                                              _C.stream_ptr(act.device)), "tsrl_sac_sample_bwd")
        return None, g_mu.to(ctx.meta[0]), g_sigma.to(ctx.meta[1])


def sac_sample(mu: torch.Tensor, sigma: torch.Tensor, eps: Optional[torch.Tensor]
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(tanh(mu + eps * sigma) [b, A], its corrected log-probability [b]) with gradients
    towards mu and sigma; ``eps`` None is the deterministic action."""
    return _SacSample.apply(eps, mu, sigma)


def sac_target_device(q1: torch.Tensor, q2: torch.Tensor, log_prob: torch.Tensor,
                      alpha: torch.Tensor) -> torch.Tensor:
    """sac.py:141-144: min(q1, q2) - alpha * log_prob over [b] rows, alpha a one-element f32
    device tensor; the result has q1's shape."""
    a, c, lp = _rows(q1).view(-1), _rows(q2).view(-1), _rows(log_prob).view(-1)
    if not a.numel() == c.numel() == lp.numel() or alpha.numel() != 1:
        raise ValueError("sac_target_device: q1, q2 and log_prob need one length, alpha one "
                         "element")
    out = torch.empty_like(a)
    _C.check(_C.lib().tsrl_sac_target(_C.ptr(a), _C.ptr(c), _C.ptr(lp),
                                      _C.ptr(alpha, torch.float32), a.numel(), _C.ptr(out),
                                      _C.stream_ptr(a.device)), "tsrl_sac_target")
    return out.view(q1.shape)


class _SacActorLoss(KernelGradLoss):
    """sac.py:162-165 and 171-173 as tsrl_sac_actor_loss_fwd_bwd.  The output is the handle to
    call backward on (towards q1, q2 and log_prob); the losses go to ``loss`` and the
    temperature's gradient to ``g_log_alpha`` (see sac_actor_loss)."""

    @staticmethod
    def forward(ctx, args, q1, q2, log_prob):
        alpha, log_alpha, target_entropy, loss, g_log_alpha = args
        xs = [_rows(t).view(-1) for t in (q1, q2, log_prob)]
        b, dev = xs[0].numel(), xs[0].device
        if not all(t.numel() == b for t in xs) or alpha.numel() != 1 or loss.numel() != (
                1 if log_alpha is None else 2):
            raise ValueError(f"_SacActorLoss: q1, q2 and log_prob need {b} elements each, "
                             "alpha one, loss one (two with log_alpha)")
        grads = [torch.empty_like(t) for t in xs]
        _C.check(_C.lib().tsrl_sac_actor_loss_fwd_bwd(
            *(_C.ptr(t) for t in xs), _C.ptr(alpha, torch.float32),
            _C.ptr(log_alpha, torch.float32), float(target_entropy), b,
            *(_C.ptr(t) for t in grads), _C.ptr(_partials(b, 2, dev)),
            _C.ptr(loss, torch.float32), _C.ptr(g_log_alpha, torch.float32),
            _C.stream_ptr(dev)), "tsrl_sac_actor_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q1, q2, log_prob))
        return torch.empty((), dtype=torch.float32, device=dev)


def sac_actor_loss(q1: torch.Tensor, q2: torch.Tensor, log_prob: torch.Tensor,
                   alpha: torch.Tensor, log_alpha: Optional[torch.Tensor] = None,
                   target_entropy: float = 0.0, loss_out: Optional[torch.Tensor] = None,
                   g_log_alpha_out: Optional[torch.Tensor] = None):
    """(handle, losses, g_log_alpha): ``handle.backward()`` hands q1, q2 and log_prob the
    gradient of the actor loss mean(alpha * log_prob - min(q1, q2)) = losses[0].  With
    ``log_alpha`` (one f32 element) losses[1] is the temperature loss and g_log_alpha its
    gradient.  ``loss_out`` / ``g_log_alpha_out`` receive the outputs in place."""
    dev = q1.device
    auto = log_alpha is not None
    loss = torch.empty(2 if auto else 1, dtype=torch.float32, device=dev) if loss_out is None \
        else loss_out
    g_la = g_log_alpha_out
    if auto and g_la is None:
        g_la = torch.empty(1, dtype=torch.float32, device=dev)
    la = None if not auto else log_alpha.detach()
    handle = _SacActorLoss.apply((alpha, la, target_entropy, loss, g_la), q1, q2, log_prob)
    return handle, loss, g_la


class _SquashedGaussianMixin:
    """What SACPolicy and REDQPolicy (policy/redq.py) share on top of DDPGPolicy: the
    tanh-squashed Gaussian ``forward``, the N(0, 1) draws, the temperature as a device tensor and
    its one-parameter flat optimiser, and the graph keys that follow from them."""

    def _init_temperature(self, alpha, deterministic_eval: bool) -> None:
        """sac.py:83-94 / redq.py:87-104."""
        self._is_auto_alpha = False
        self._alpha: Union[float, torch.Tensor]
        if isinstance(alpha, tuple):
            self._is_auto_alpha = True
            self._target_entropy, self._log_alpha, self._alpha_optim = alpha
            assert alpha[1].shape == torch.Size([1]) and alpha[1].requires_grad
            self._alpha = self._log_alpha.detach().exp()
        else:
            self._alpha = alpha
        self._deterministic_eval = deterministic_eval
        self._alpha_dev = None  # ((value, device), tensor): the fixed temperature on the device
        self._alpha_fa: Optional[FlatAdam] = None

    # -- draws and temperature ------------------------------------------------------------------
    def _rsample_noise(self, shape, device) -> torch.Tensor:
        """The N(0, 1) draw of rsample (sac.py:121); every path draws through here."""
        return torch.randn(size=tuple(shape), device=device)

    def _alpha_tensor(self, dev) -> torch.Tensor:
        """The temperature as the one-element f32 device tensor the kernels read.  With
        automatic tuning it is ``_alpha`` itself, written in place by every fused update."""
        if self._is_auto_alpha:
            a = self._alpha
            if a.device != dev or a.dtype != torch.float32 or not a.is_contiguous():
                a = self._alpha = a.detach().to(device=dev, dtype=torch.float32).contiguous()
            return a
        key = (float(self._alpha), dev)
        if self._alpha_dev is None or self._alpha_dev[0] != key:
            self._alpha_dev = (key, torch.full((1,), key[0], dtype=torch.float32, device=dev))
        return self._alpha_dev[1]

    def _draws(self) -> bool:
        return not (self._deterministic_eval and not self.training)

    # -- acting ---------------------------------------------------------------------------------
    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                input: str = "obs", **kwargs: Any) -> Batch:
        """sac.py:107-135.  Fused: the actor's forward and one tsrl_sac_sample_fwd launch."""
        obs = batch[input]
        logits, hidden = self.actor(obs, state=state, info=batch.get("info", Batch()))
        assert isinstance(logits, tuple)
        mu, sigma = logits
        eps = self._rsample_noise(mu.shape, mu.device) if self._draws() else None
        if self.fused and mu.is_cuda:
            dist = Independent(Normal(mu, sigma, validate_args=False), 1, validate_args=False)
            act, log_prob = sac_sample(mu, sigma, eps)
            log_prob = log_prob.unsqueeze(-1)
        else:
            dist = Independent(Normal(*logits), 1)
            raw = mu if eps is None else mu + eps.to(mu.dtype) * sigma  # rsample
            log_prob = dist.log_prob(raw).unsqueeze(-1)
            act = torch.tanh(raw)
            log_prob = log_prob - torch.log((1 - act.pow(2)) + EPS32).sum(-1, keepdim=True)
        return Batch(logits=logits, act=act, state=hidden, dist=dist, log_prob=log_prob)

    def _bind_alpha(self) -> Optional[FlatAdam]:
        """The one-parameter flat storage of ``log_alpha`` when ``alpha_optim`` is a plain
        Adam / RMSprop over it (None: torch's step, and no graph)."""
        if not (self._is_auto_alpha and self.fused and self.fused_adam
                and self._log_alpha.is_cuda and self._log_alpha.dtype == torch.float32):
            return None
        if self._alpha_fa is None:
            self._alpha_fa = FlatAdam([self._log_alpha])
        fa = self._alpha_fa
        if not fa.bind_adam(self._alpha_optim):
            return None
        fa.bind_grads()
        fa.set_lr()
        return fa

    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        """sac.py:147-190 / redq.py:159-200; see DDPGPolicy.learn."""
        self._bind_alpha()
        return super().learn(batch, **kwargs)

    def _learn_draws(self, act: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        if not self._draws():
            return ()
        return (_rows(self._rsample_noise(act.shape, act.device)),)

    def _alpha_flat(self) -> Optional[FlatAdam]:
        """log_alpha's flat storage while it serves ``alpha_optim``, else None."""
        fa = self._alpha_fa
        return fa if fa is not None and fa.adam_bound(self._alpha_optim) else None

    def _graph_ok(self, obs, n: int) -> bool:
        if self._is_auto_alpha and self._alpha_flat() is None:
            return False
        return super()._graph_ok(obs, n)

    def _graph_addr(self, fas) -> tuple:
        addr = super()._graph_addr(fas)
        dev = next(self.actor.parameters()).device
        extra = [self._alpha_tensor(dev).data_ptr()]
        if self._is_auto_alpha:
            extra += [self._log_alpha.data_ptr(), self._alpha_fa.flat_grad.data_ptr()]
        return addr + (tuple(extra),)

    def _alpha_step(self, g_la: torch.Tensor, alpha: torch.Tensor) -> None:
        """The temperature's optimiser pass on the loss kernel's gradient ``g_la`` and alpha =
        exp(log_alpha) in place (sac.py:174-177)."""
        fa = self._alpha_flat()
        if fa is not None:  # the gradient landed in log_alpha's flat .grad
            fa.clip_adam(None)
            torch.exp(self._log_alpha.detach(), out=alpha)
        else:  # another optimiser: torch's step on the kernel's gradient
            self._alpha_optim.zero_grad()
            self._log_alpha.grad = g_la.to(self._log_alpha.dtype).view_as(self._log_alpha)
            self._alpha_optim.step()
            alpha.copy_(self._log_alpha.detach().exp())


class SACPolicy(_SquashedGaussianMixin, DDPGPolicy):
    """Constructor arguments, defaults and assertions as the reference's (sac.py:54-94); the
    device-path attributes are DDPGPolicy's."""

    _critic_names = ("critic1", "critic2")
    _sync_order = ("critic1", "critic2")  # sac.py:103-105: the actor has no target copy
    _optim_order = ("critic1", "critic2", "actor")
    # the Collector keeps this policy on its eager device step: every forward draws
    eager_collect_step = True

    def __init__(self, actor: torch.nn.Module, actor_optim: torch.optim.Optimizer,
                 critic1: torch.nn.Module, critic1_optim: torch.optim.Optimizer,
                 critic2: torch.nn.Module, critic2_optim: torch.optim.Optimizer,
                 tau: float = 0.005, gamma: float = 0.99,
                 alpha: Union[float, Tuple[float, torch.Tensor, torch.optim.Optimizer]] = 0.2,
                 reward_normalization: bool = False, estimation_step: int = 1,
                 exploration_noise: Optional[BaseNoise] = None,
                 deterministic_eval: bool = True, **kwargs: Any) -> None:
        super().__init__(None, None, None, None, tau, gamma, exploration_noise,
                         reward_normalization, estimation_step, **kwargs)
        self.actor, self.actor_optim = actor, actor_optim
        self.critic1, self.critic1_old = critic1, deepcopy(critic1)
        self.critic1_old.eval()
        self.critic1_optim = critic1_optim
        self.critic2, self.critic2_old = critic2, deepcopy(critic2)
        self.critic2_old.eval()
        self.critic2_optim = critic2_optim
        self._init_temperature(alpha, deterministic_eval)

    # -- process_fn -----------------------------------------------------------------------------
    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """sac.py:137-145: min over the target critics at the sampled next action, less
        alpha times its log-probability."""
        obs_next = self._obs_next(buffer, indices)
        res = self(Batch(obs_next=obs_next, info=Batch()), input="obs_next")
        q1, q2 = self.critic1_old(obs_next, res.act), self.critic2_old(obs_next, res.act)
        if self.fused and q1.is_cuda:
            return sac_target_device(q1, q2, res.log_prob, self._alpha_tensor(q1.device))
        return torch.min(q1, q2) - self._alpha * res.log_prob

    # -- learn ----------------------------------------------------------------------------------
    def _loss_slots(self) -> int:
        return 5 if self._is_auto_alpha else 3  # critics, actor (, temperature loss, alpha)

    def _result(self, losses: List[float], did_actor: bool) -> Dict[str, float]:
        """sac.py:181-190."""
        result = {"loss/actor": losses[2], "loss/critic1": losses[0], "loss/critic2": losses[1]}
        if self._is_auto_alpha:
            result["loss/alpha"] = losses[3]
            result["alpha"] = losses[4]
        return result

    def _learn_torch(self, batch: Batch, do_actor: bool):
        """The reference's op sequence as written (sac.py:147-179)."""
        td1, critic1_loss = self._mse_optimizer(batch, self.critic1, self.critic1_optim)
        td2, critic2_loss = self._mse_optimizer(batch, self.critic2, self.critic2_optim)
        td = ((td1 + td2) / 2.0).detach()
        obs_result = self(batch)
        act = obs_result.act
        current_q1a = self.critic1(batch.obs, act).flatten()
        current_q2a = self.critic2(batch.obs, act).flatten()
        actor_loss = (self._alpha * obs_result.log_prob.flatten()
                      - torch.min(current_q1a, current_q2a)).mean()
        self.actor_optim.zero_grad()
        actor_loss.backward()
        self.actor_optim.step()
        losses = [critic1_loss.detach(), critic2_loss.detach(), actor_loss.detach()]
        if self._is_auto_alpha:
            log_prob = obs_result.log_prob.detach() + self._target_entropy
            alpha_loss = -(self._log_alpha * log_prob).mean()
            self._alpha_optim.zero_grad()
            alpha_loss.backward()
            self._alpha_optim.step()
            self._alpha = self._log_alpha.detach().exp()
            losses += [alpha_loss.detach(), self._alpha.reshape(())]
        self.sync_weight()
        return torch.stack([t.to(torch.float32) for t in losses]), td

    def _step(self, fas, obs, act, returns, weight, do_actor: bool, td_out: torch.Tensor,
              loss_out: torch.Tensor, eps: Optional[torch.Tensor] = None) -> None:
        """One update (sac.py:147-179): both critics' forward, their fused losses, backward
        and optimiser passes; the actor's forward, the sample kernel, both critics at the
        sampled action, the fused actor / temperature loss, backward into the actor alone and
        its optimiser pass; the temperature's optimiser pass and alpha = exp(log_alpha) in
        place; the soft update.  loss_out: critic1, critic2, actor (, temperature loss,
        alpha)."""
        names = self._critic_names
        qs = [getattr(self, name)(obs, act).flatten() for name in names]
        handle, _, _ = q_mse_loss(qs, returns, weight, td_out, loss_out[:2])
        self._backward_step(handle, names, fas)
        (mu, sigma), _ = self.actor(obs, state=None, info=Batch())
        a, log_prob = sac_sample(mu, sigma, eps)
        q1a, q2a = self.critic1(obs, a).flatten(), self.critic2(obs, a).flatten()
        alpha = self._alpha_tensor(a.device)
        if not self._is_auto_alpha:
            handle, _, _ = sac_actor_loss(q1a, q2a, log_prob, alpha, loss_out=loss_out[2:3])
            self._backward_step(handle, ("actor",), fas)
            self.sync_weight()
            return
        fa = self._alpha_flat()
        handle, _, g_la = sac_actor_loss(
            q1a, q2a, log_prob, alpha, self._log_alpha, self._target_entropy, loss_out[2:4],
            None if fa is None else fa.flat_grad)  # the gradient lands in log_alpha's .grad
        self._backward_step(handle, ("actor",), fas)
        self._alpha_step(g_la, alpha)
        loss_out[4:5].copy_(alpha)
        self.sync_weight()
