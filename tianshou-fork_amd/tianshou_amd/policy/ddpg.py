"""DDPGPolicy (tianshou/policy/modelfree/ddpg.py:44-204): deterministic policy gradient with
n-step targets, Polyak-averaged target networks and additive exploration noise, on the device
path.  TD3Policy (policy/td3.py) fills the class attributes and hooks below.

The actor and the critics stay torch modules (utils/net.py ``Actor`` / ``Critic``).  Around
their forwards an update is launch-latency work on a few hundred rows, so the glue runs as the
kernels of csrc/ddpg.hip: ``tsrl_q_mse_fwd_bwd`` (every critic's TD error, loss and gradient in
one pass), ``tsrl_neg_mean_fwd_bwd`` (the actor loss), ``tsrl_soft_update`` (sync_weight over
all networks in one launch) and ``tsrl_act_noise`` (exploration_noise over NumPy's draws).
With plain Adam / RMSprop optimisers every network's parameters, gradients and moments live in
flat buffers (policy/flat_adam.py, one FlatAdam per network), its target network's parameters
are views into a second flat buffer laid out as the first, and "critic forward, loss, backward,
optimiser pass, actor forward, critic forward, loss, backward, optimiser pass, soft update"
replays from one captured HIP graph (``graph_learn``).  The target mirror, the bracket around
each backward and the graph cache are policy/flat_learn.py's, shared with DQNPolicy.

What stays on torch: a network with module buffers or another optimiser (``soft_update`` /
``optim.step()`` for that network; no graph replay), and ``fused = False`` -- the reference's
op sequence on the GPU, kept as the comparison leg of tools/ddpg_update_bench.py.

SACPolicy (policy/sac.py), DiscreteSACPolicy (policy/discrete_sac.py) and REDQPolicy
(policy/redq.py) build on the same hooks; OffpolicyTrainer (trainer/base.py) drives them all.
Not built: data-parallel updates, a fused act kernel for deterministic actors (the Collector
keeps such a policy on its eager device step) and reward normalisation (compute_nstep_return
asserts against it).
"""
import warnings
from copy import deepcopy
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.exploration import BaseNoise, GaussianNoise
from tianshou_amd.policy.base import BasePolicy
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import (KernelGradLoss, _partials, _unit_seed, f32_rows,
                                            flat_backward, mirror_target, replay_learn_graph,
                                            target_mirrored)
from tianshou_amd.utils.capture import graph_capture

SOFT_UPDATE_MAX_SEGMENTS = 4


def soft_update_device(pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]], tau: float) -> None:
    """target = tau * source + (1 - tau) * target for every (target, source) pair of contiguous
    f32 device tensors, four pairs per tsrl_soft_update launch."""
    pairs = list(pairs)
    for t, s in pairs:
        if t.numel() != s.numel() or t.dtype != torch.float32 or s.dtype != torch.float32:
            raise ValueError("soft_update_device: each pair needs two f32 tensors of one size")
    for o in range(0, len(pairs), SOFT_UPDATE_MAX_SEGMENTS):
        args: List[Any] = []
        for t, s in pairs[o:o + SOFT_UPDATE_MAX_SEGMENTS]:
            args += [_C.ptr(t), _C.ptr(s), t.numel()]
        args += [None, None, 0] * (SOFT_UPDATE_MAX_SEGMENTS - len(args) // 3)
        _C.check(_C.lib().tsrl_soft_update(*args, float(tau),
                                           _C.stream_ptr(pairs[o][0].device)),
                 "tsrl_soft_update")


def act_noise_device(act: torch.Tensor, noise: np.ndarray) -> torch.Tensor:
    """(act.astype(f64) + noise).astype(f32) on the device: ``noise`` is the host's f64 draw."""
    a = act.detach().to(torch.float32).contiguous()
    z = torch.as_tensor(np.array(np.broadcast_to(noise, tuple(a.shape)), dtype=np.float64),
                        device=a.device)
    out = torch.empty_like(a)
    _C.check(_C.lib().tsrl_act_noise(_C.ptr(a), _C.ptr(z), a.numel(), _C.ptr(out),
                                     _C.stream_ptr(a.device)), "tsrl_act_noise")
    return out


class _QMSELoss(KernelGradLoss):
    """ddpg.py:173-178 for one or two critics as tsrl_q_mse_fwd_bwd.  The output is the sum of
    the critics' losses, the handle to call backward on; the per-critic losses and the per-row
    vector are written to ``loss`` / ``td`` (see q_mse_loss)."""

    @staticmethod
    def forward(ctx, args, *qs):
        returns, weight, td, loss = args
        dev = qs[0].device
        x = [q.detach().float().contiguous() for q in qs]
        b = x[0].numel()
        if not 1 <= len(x) <= 2 or loss.numel() != len(x) or not all(
                t is None or t.numel() == b for t in (*x, returns, weight, td)):
            raise ValueError(f"_QMSELoss: one or two critics' q, returns, weight and td need {b} "
                             "elements each, loss one per critic")
        grads = [torch.empty_like(t) for t in x]
        total = torch.empty((), dtype=torch.float32, device=dev)
        _C.check(_C.lib().tsrl_q_mse_fwd_bwd(
            _C.ptr(x[0]), _C.ptr(x[1]) if len(x) > 1 else None,
            _C.ptr(returns, torch.float32), _C.ptr(weight, torch.float32), b, _C.ptr(grads[0]),
            _C.ptr(grads[1]) if len(x) > 1 else None, _C.ptr(td, torch.float32),
            _C.ptr(_partials(b, 2, dev)), _C.ptr(loss, torch.float32), _C.ptr(total),
            _C.stream_ptr(dev)), "tsrl_q_mse_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, qs)
        return total


def q_mse_loss(qs: Sequence[torch.Tensor], returns: torch.Tensor,
               weight: Optional[torch.Tensor], td_out: Optional[torch.Tensor] = None,
               loss_out: Optional[torch.Tensor] = None):
    """(handle, losses [len(qs)], per-row vector [b]) of the critics' outputs ``qs`` ([b] each):
    ``handle.backward()`` hands every critic the gradient of its own loss.  ``td_out`` /
    ``loss_out`` receive the outputs in place (the static outputs of a captured graph)."""
    dev, b = qs[0].device, qs[0].numel()
    td = torch.empty(b, dtype=torch.float32, device=dev) if td_out is None else td_out
    loss = torch.empty(len(qs), dtype=torch.float32, device=dev) if loss_out is None \
        else loss_out
    return _QMSELoss.apply((returns, weight, td, loss), *qs), loss, td


class _NegMeanLoss(KernelGradLoss):
    """ddpg.py:189's -Q.mean() as tsrl_neg_mean_fwd_bwd; with ``loss_out`` the loss goes there
    and the output is only the handle to call backward on."""

    @staticmethod
    def forward(ctx, loss_out, q):
        x = q.detach().float().contiguous()
        b, dev = x.numel(), x.device
        grad = torch.empty_like(x)
        handle = torch.empty((), dtype=torch.float32, device=dev)
        loss = handle if loss_out is None else loss_out
        if loss.numel() != 1:
            raise ValueError("_NegMeanLoss: loss_out needs one element")
        _C.check(_C.lib().tsrl_neg_mean_fwd_bwd(
            _C.ptr(x), b, _C.ptr(grad), _C.ptr(_partials(b, 1, dev)),
            _C.ptr(loss, torch.float32), _C.stream_ptr(dev)), "tsrl_neg_mean_fwd_bwd")
        KernelGradLoss.keep(ctx, (grad,), (q,))
        return handle


def neg_mean_loss(q: torch.Tensor, loss_out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-mean(q) with gradient -1/b.  Without ``loss_out`` the result is the loss; with it the
    loss is written there and the result is the backward handle alone."""
    return _NegMeanLoss.apply(loss_out, q)


class DDPGPolicy(BasePolicy):
    """Constructor arguments, defaults, assertions and warnings as the reference's
    (ddpg.py:44-104).

    Attributes that select the device paths, read as on DQNPolicy: ``fused`` (False: the
    reference's torch formulation throughout), ``fused_adam`` (False: keep ``optim.step()`` and
    ``soft_update`` even for a plain Adam / RMSprop) and ``graph_learn`` (None / True / False:
    None replays updates of fewer than GRAPH_LEARN_MAX_ROWS rows)."""

    _critic_names: Tuple[str, ...] = ("critic",)
    # the networks with a target copy, in sync_weight's order (ddpg.py:119-120)
    _sync_order: Tuple[str, ...] = ("actor", "critic")

    @property
    def _optim_order(self) -> Tuple[str, ...]:
        """The networks with an optimiser of their own.  Here and in TD3Policy every one of
        them has a target copy too; SACPolicy's actor has none."""
        return self._sync_order

    def __init__(self, actor: Optional[torch.nn.Module],
                 actor_optim: Optional[torch.optim.Optimizer],
                 critic: Optional[torch.nn.Module],
                 critic_optim: Optional[torch.optim.Optimizer], tau: float = 0.005,
                 gamma: float = 0.99,
                 exploration_noise: Optional[BaseNoise] = GaussianNoise(sigma=0.1),
                 reward_normalization: bool = False, estimation_step: int = 1,
                 action_scaling: bool = True, action_bound_method: Optional[str] = "clip",
                 **kwargs: Any) -> None:
        super().__init__(action_scaling=action_scaling, action_bound_method=action_bound_method,
                         **kwargs)
        assert action_bound_method != "tanh", (
            "tanh mapping is not supported in policies where action is used as input of "
            "critic, because raw action in range (-inf, inf) will cause instability in training")
        try:
            if actor is not None and action_scaling and not np.isclose(actor.max_action, 1.0):
                warnings.warn(
                    "action_scaling and action_bound_method are only intended to deal with "
                    "unbounded model action space, but find actor model bound action space "
                    f"with max_action={actor.max_action}. Consider using unbounded=True option "
                    "of the actor model, or set action_scaling to False and "
                    'action_bound_method to "".')
        except Exception:
            pass
        if actor is not None and actor_optim is not None:
            self.actor = actor
            self.actor_old = deepcopy(actor)
            self.actor_old.eval()
            self.actor_optim = actor_optim
        if critic is not None and critic_optim is not None:
            self.critic = critic
            self.critic_old = deepcopy(critic)
            self.critic_old.eval()
            self.critic_optim = critic_optim
        assert 0.0 <= tau <= 1.0, "tau should be in [0, 1]"
        self.tau = tau
        assert 0.0 <= gamma <= 1.0, "gamma should be in [0, 1]"
        self._gamma = gamma
        self._noise = exploration_noise
        self._rew_norm = reward_normalization
        self._n_step = estimation_step
        self.fused = True
        self.fused_adam = True
        self.graph_learn = None
        self._graph_failed = False
        self._learn_graphs: Dict[Any, dict] = {}
        self._flats: Dict[str, dict] = {}
        self._warm = False

    def set_exp_noise(self, noise: Optional[BaseNoise]) -> None:
        self._noise = noise

    def train(self, mode: bool = True) -> "DDPGPolicy":
        """ddpg.py:110-115: the target networks stay in eval mode."""
        self.training = mode
        for name in self._optim_order:
            getattr(self, name).train(mode)
        return self

    # -- flat parameter storage -----------------------------------------------------------------
    def _on_device(self) -> bool:
        p = next(self.actor.parameters(), None)
        return p is not None and p.is_cuda

    def _bind(self, name: str) -> Optional[FlatAdam]:
        """The flat gradient / optimiser storage of network ``name`` when its optimiser is a
        plain Adam or RMSprop over exactly its parameters (None otherwise: torch's step and
        BasePolicy.soft_update run for it).  Its target network's parameters, where it has one,
        then become views into a second flat buffer (flat_learn.mirror_target)."""
        if not (self.fused and self.fused_adam and self._on_device()):
            return None
        net, old = getattr(self, name), getattr(self, name + "_old", None)
        st = self._flats.get(name)
        if st is None:
            st = self._flats[name] = dict(fa=FlatAdam(net.parameters()), old=None, src=None)
        fa = st["fa"]
        if not fa.bind_adam(getattr(self, name + "_optim")):
            st["old"] = st["src"] = None
            return None
        if old is not None and not self._old_is_flat(st, old):
            st["src"] = fa.flat_param
            st["old"] = mirror_target(old, fa.params, st["src"])
        return fa

    @staticmethod
    def _old_is_flat(st: dict, old: torch.nn.Module) -> bool:
        return target_mirrored(old, st["old"], st["src"], st["fa"].flat_param)

    def _flat_pair(self, name: str) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(flat target, flat online) parameters of network ``name`` when tsrl_soft_update can
        serve it: flat storage bound on both sides and no module buffers."""
        st = self._flats.get(name)
        if not self.fused or st is None:
            return None
        net, old = getattr(self, name), getattr(self, name + "_old")
        if st["fa"].adam_bound(getattr(self, name + "_optim")) and self._old_is_flat(st, old) \
                and next(net.buffers(), None) is None:
            return st["old"], st["fa"].flat_param
        return None

    def _flat_ready(self, name: str) -> bool:
        """Network ``name`` steps and (where it has a target copy) syncs on flat storage alone:
        what a captured update needs of every network."""
        if hasattr(self, name + "_old"):
            return self._flat_pair(name) is not None
        st = self._flats.get(name)
        return bool(self.fused and st is not None
                    and st["fa"].adam_bound(getattr(self, name + "_optim"))
                    and next(getattr(self, name).buffers(), None) is None)

    def sync_weight(self) -> None:
        """ddpg.py:117-120 (td3.py:93-96): every network with flat storage in one
        tsrl_soft_update launch, any other through BasePolicy.soft_update."""
        pairs = []
        for name in self._sync_order:
            pair = self._flat_pair(name)
            if pair is None:
                self.soft_update(getattr(self, name + "_old"), getattr(self, name), self.tau)
            else:
                pairs.append(pair)
        if pairs:
            soft_update_device(pairs, self.tau)

    # -- acting ---------------------------------------------------------------------------------
    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                model: str = "actor", input: str = "obs", **kwargs: Any) -> Batch:
        """ddpg.py:143-166."""
        net = getattr(self, model)
        actions, hidden = net(batch[input], state=state, info=batch.get("info", Batch()))
        return Batch(act=actions, state=hidden)

    def exploration_noise(self, act, batch: Batch):
        """ddpg.py:196-204.  The draw comes from the host noise process (NumPy's global stream,
        the reference's shapes and order).  A NumPy ``act`` stays on the host; for a device
        ``act`` the f64 draw is uploaded and added by tsrl_act_noise, the f64 sum rounded to
        the f32 that this package's buffer and the critic's forward use."""
        if self._noise is None:
            return act
        if isinstance(act, np.ndarray):
            return act + self._noise(act.shape)
        if isinstance(act, torch.Tensor):
            noise = self._noise(tuple(act.shape))
            if act.is_cuda:
                return act_noise_device(act, noise)
            return torch.as_tensor((act.detach().numpy().astype(np.float64) + noise)
                                   .astype(np.float32))
        warnings.warn("Cannot add exploration noise to non-numpy_array action.")
        return act

    # -- process_fn -----------------------------------------------------------------------------
    @staticmethod
    def _obs_next(buffer, indices: np.ndarray):
        return buffer.get(indices, "obs_next") if getattr(buffer, "_save_obs_next", True) \
            else buffer[indices].obs_next

    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """ddpg.py:122-127: Q_target(s_{t+n}, actor_target(s_{t+n}))."""
        obs_next = self._obs_next(buffer, indices)
        batch = Batch(obs_next=obs_next, info=Batch())
        act_ = self(batch, model="actor_old", input="obs_next").act
        return self.critic_old(obs_next, act_)

    def process_fn(self, batch: Batch, buffer, indices: np.ndarray) -> Batch:
        """ddpg.py:129-141: n-step returns over the buffer (tsrl_nstep_return)."""
        return self.compute_nstep_return(batch, buffer, indices, self._target_q, self._gamma,
                                         self._n_step, self._rew_norm)

    # -- learn ----------------------------------------------------------------------------------
    @staticmethod
    def _mse_optimizer(batch: Batch, critic: torch.nn.Module,
                       optimizer: torch.optim.Optimizer) -> Tuple[torch.Tensor, torch.Tensor]:
        """ddpg.py:168-182 as written."""
        weight = batch.get("weight", None)
        current_q = critic(batch.obs, batch.act).flatten()
        target_q = torch.as_tensor(batch.returns, device=current_q.device).flatten()
        td = current_q - target_q
        if weight is None:
            weight = 1.0
        elif not isinstance(weight, float):
            weight = torch.as_tensor(weight, device=td.device).to(td.dtype)
        critic_loss = (td.pow(2) * weight).mean()
        optimizer.zero_grad()
        critic_loss.backward()
        optimizer.step()
        return td, critic_loss

    def _actor_step_due(self) -> bool:
        return True

    def _result(self, losses: List[float], did_actor: bool) -> Dict[str, float]:
        return {"loss/actor": losses[-1], "loss/critic": losses[0]}

    def _loss_slots(self) -> int:
        """Length of the device vector that the update's one host read brings back: one loss
        per critic, then the actor's."""
        return len(self._critic_names) + 1

    def _learn_draws(self, act: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        """Random draws of one fused update, made before it runs: further static inputs of a
        captured graph, handed to _step after its other arguments.  None here."""
        return ()

    def _learn_act(self, batch: Batch, dev, n: int) -> torch.Tensor:
        """``batch.act`` as the fused update takes it: f32 [n, act_dim] here; the int64 [n]
        indices of DiscreteSACPolicy."""
        return torch.as_tensor(batch.act, device=dev).to(torch.float32).reshape(n, -1) \
            .contiguous()

    def _learn_torch(self, batch: Batch, do_actor: bool):
        """The reference's op sequence as written (ddpg.py:184-194, td3.py:111-128), on
        whatever device the networks live on; returns (losses, per-row vector)."""
        tds, losses = [], []
        for name in self._critic_names:
            td, loss = self._mse_optimizer(batch, getattr(self, name),
                                           getattr(self, name + "_optim"))
            tds.append(td.detach())
            losses.append(loss.detach())
        td = tds[0] if len(tds) == 1 else (tds[0] + tds[1]) / 2.0
        if do_actor:
            critic = getattr(self, self._critic_names[0])
            actor_loss = -critic(batch.obs, self(batch).act).mean()
            self.actor_optim.zero_grad()
            actor_loss.backward()
            losses.append(actor_loss.detach())
            self.actor_optim.step()
            self.sync_weight()
        return torch.stack(losses), td

    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        """ddpg.py:184-194.  ``batch.weight`` leaves as the detached device TD error (what a
        prioritized buffer's update_weight takes); all losses come back in the update's one
        host read."""
        do_actor = self._actor_step_due()
        nc = len(self._critic_names)
        if not (self.fused and self._on_device()):
            loss, td = self._learn_torch(batch, do_actor)
        else:
            fas = {name: self._bind(name) for name in self._optim_order}
            dev = next(self.actor.parameters()).device
            n = len(batch.returns)
            weight = batch.get("weight", None)
            obs = batch.obs
            act = self._learn_act(batch, dev, n)
            returns = f32_rows(batch.returns, dev, n)
            w = None if weight is None else f32_rows(weight, dev, n)
            draws = self._learn_draws(act)
            out = None
            if all(fa is not None for fa in fas.values()):
                for fa in fas.values():
                    fa.set_lr()
                if self._warm and self._graph_ok(obs, n):
                    out = self._graph_step(fas, obs, act, returns, w, do_actor, *draws)
            if out is None:
                loss = torch.empty(self._loss_slots(), dtype=torch.float32, device=dev)
                td = torch.empty(n, dtype=torch.float32, device=dev)
                self._step(fas, obs, act, returns, w, do_actor, td, loss, *draws)
                out = (loss, td)
            loss, td = out
            self._warm = True
        batch.weight = td.detach()  # prio-buffer
        vals = loss.tolist()
        return self._result(vals if do_actor else vals[:nc], do_actor)

    def _backward_step(self, handle: torch.Tensor, names: Sequence[str],
                       fas: Dict[str, Optional[FlatAdam]]) -> None:
        """zero_grad, backward and optimiser step of networks ``names`` on loss ``handle``.
        Only their parameters receive gradients: the actor loss's backward runs through the
        critic without leaving anything in the critic's gradient storage."""
        params = []
        for name in names:
            if fas[name] is None:
                getattr(self, name + "_optim").zero_grad()
            params += list(getattr(self, name).parameters())
        with flat_backward([fas[name] for name in names if fas[name] is not None]):
            torch.autograd.backward(handle, _unit_seed(handle.device), inputs=params)
        for name in names:
            fa = fas[name]
            if fa is None:
                getattr(self, name + "_optim").step()
            else:
                fa.clip_adam(None)  # the reference clips nothing: one optimiser pass

    def _step(self, fas: Dict[str, Optional[FlatAdam]], obs, act, returns, weight,
              do_actor: bool, td_out: torch.Tensor, loss_out: torch.Tensor) -> None:
        """One update: every critic's forward, their fused losses, backward and optimiser
        passes; then (``do_actor``) the actor step through the first critic and the soft
        update.  The critics are independent networks, so forwarding all of them before
        stepping any gives what stepping them one after the other gives.  loss_out: one loss
        per critic, then the actor's."""
        names = self._critic_names
        qs = [getattr(self, name)(obs, act).flatten() for name in names]
        handle, _, _ = q_mse_loss(qs, returns, weight, td_out, loss_out[:len(names)])
        self._backward_step(handle, names, fas)
        if not do_actor:
            return
        a, _ = self.actor(obs, state=None, info=Batch())
        q = getattr(self, names[0])(obs, a).flatten()
        handle = neg_mean_loss(q, loss_out[len(names):])
        self._backward_step(handle, ("actor",), fas)
        self.sync_weight()

    # -- HIP-graph replay of one update ----------------------------------------------------------
    def _graph_ok(self, obs, n: int) -> bool:
        if self._graph_failed or not isinstance(obs, torch.Tensor) or not obs.is_cuda:
            return False
        return self._use_graph(n) and all(self._flat_ready(name) for name in self._optim_order)

    def _capture(self, graph):
        """The capture context of a learn graph (utils.capture.graph_capture)."""
        return graph_capture(graph)

    def _graph_addr(self, fas: Dict[str, FlatAdam]) -> tuple:
        """The flat addresses a captured update is tied to."""
        addr = []
        for name in self._optim_order:
            fa = fas[name]
            fa.bind_grads()
            old = self._flats[name]["old"]
            addr.append((fa.flat_grad.data_ptr(), None if old is None else old.data_ptr(),
                         tuple(p.data_ptr() for p in fa.params)))
        return tuple(addr)

    def _graph_step(self, fas: Dict[str, FlatAdam], obs, act, returns, weight, do_actor: bool,
                    *draws: torch.Tensor):
        """One update replayed from a HIP graph captured once per (batch size, observation
        shape and dtype, action shape, weight present, step kind, draws, flat addresses);
        static copies of obs / act / returns / weight / the draws feed it, the losses and the
        per-row vector come out of static outputs (flat_learn.replay_learn_graph).  None if the
        capture failed (this and every later update then run eagerly)."""
        addr = self._graph_addr(fas)
        key = (len(returns), tuple(obs.shape), obs.dtype, tuple(act.shape), weight is not None,
               *(tuple(d.shape) for d in draws), bool(do_actor))
        out = replay_learn_graph(
            self._learn_graphs, key, addr, (obs, act, returns, weight, *draws),
            lambda: (torch.empty(len(returns), dtype=torch.float32, device=act.device),
                     torch.zeros(self._loss_slots(), dtype=torch.float32, device=act.device)),
            lambda s, td, loss: self._step(fas, *s[:4], do_actor, td, loss, *s[4:]),
            self._capture)
        if out is None:
            self._graph_failed = True
        return out
