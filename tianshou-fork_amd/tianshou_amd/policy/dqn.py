"""DQNPolicy (tianshou/policy/modelfree/dqn.py:11-203): Nature DQN / double DQN with n-step
targets, an optional hard-synced target network and epsilon-greedy exploration, on the device
path.

The Q-network stays a torch module (utils/net.py ``Net``, utils/net_atari.py ``DQN``).  Around
its forwards the update is launch-latency work on 32 to a few hundred rows, so the glue runs
as the kernels of csrc/dqn.hip: ``tsrl_dqn_target_q`` (the bootstrap value of ``_target_q``),
``tsrl_dqn_td_fwd_bwd`` (learn()'s TD error, loss and gradient in one pass) and
``tsrl_eps_greedy`` (exploration_noise over NumPy's draws).  With a plain Adam or RMSprop the
parameters, gradients and moments live in flat buffers (policy/flat_adam.py): the optimiser
step is one HIP pass, the target network's parameters are views into a second flat buffer
(``sync_weight`` is one copy), and "forward, loss, backward, optimiser pass" can replay from
a captured HIP graph (``graph_learn``).  The target mirror, the bracket around the backward
call and the per-key graph cache are policy/flat_learn.py's, shared with DDPGPolicy.

What stays on torch: observations with an action mask (``obs.mask``), any other optimiser
(``optim.step()``), and ``fused = False`` -- the reference's op sequence on the GPU, kept as
the comparison leg of tools/dqn_update_bench.py.

The distributional subclasses C51Policy (policy/c51.py) and QRDQNPolicy (policy/qrdqn.py) fill
the hooks below (``_greedy_act``, ``_learn_inputs``, ``_returns_rows``, ``_loss_weight``,
``_before_forward``, ``_forward_q``, ``_fused_loss``) and reuse the flat storage, the sync and
the graph replay as they are; RainbowPolicy (policy/rainbow.py) is C51Policy over NoisyLinear
layers, IQNPolicy (policy/iqn.py) QRDQNPolicy over ImplicitQuantileNetwork, and FQFPolicy
(policy/fqf.py) adds a second network with a flat optimiser of its own (``_flats``,
``_loss_out``, ``_learn_result``).  BranchingDQNPolicy (policy/bdq.py) has [b, K] actions
(``_learn_act``) and a target and a loss of its own.
"""
from copy import deepcopy
from typing import Any, Dict, Optional, Union

import numpy as np
import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.base import BasePolicy
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import (f32_rows, flat_backward, mirror_target,
                                            replay_learn_graph, target_mirrored)
from tianshou_amd.policy.onpolicy import _is_unit_seed, _unit_seed
from tianshou_amd.utils.capture import graph_capture


def target_q_device(q_sel: Optional[torch.Tensor], q_eval: torch.Tensor, is_double: bool
                    ) -> torch.Tensor:
    """dqn.py:93-96 as one launch: q_eval[r, argmax q_sel[r]] (double) or max q_eval[r]."""
    q_eval = q_eval.detach().float().contiguous()
    if is_double:
        q_sel = q_eval if q_sel is None else q_sel.detach().float().contiguous()
    b, A = q_eval.shape
    if is_double and q_sel.shape != q_eval.shape:
        raise ValueError(f"target_q_device: q_sel {tuple(q_sel.shape)} != q_eval {(b, A)}")
    out = torch.empty(b, dtype=torch.float32, device=q_eval.device)
    _C.check(_C.lib().tsrl_dqn_target_q(_C.ptr(q_sel) if is_double else None, _C.ptr(q_eval), b,
                                        A, int(bool(is_double)), _C.ptr(out),
                                        _C.stream_ptr(q_eval.device)), "tsrl_dqn_target_q")
    return out


class _DQNLoss(torch.autograd.Function):
    """dqn.py:172-185 as tsrl_dqn_td_fwd_bwd: q is the network's [b, A] output; returns
    (loss, td_error).  ``td_out`` / ``loss_out`` (optional) receive the outputs in place: the
    static outputs of a captured graph."""

    @staticmethod
    def forward(ctx, q, ctx_args):
        act, returns, weight, huber, td_out, loss_out = ctx_args
        dev = q.device
        x = q.detach().float().contiguous()
        b, A = x.shape
        if not all(t is None or t.numel() == b for t in (act, returns, weight, td_out)):
            raise ValueError(f"_DQNLoss: act / returns / weight / td_out need {b} elements")
        L = _C.lib()
        grad_q = torch.empty_like(x)
        td = torch.empty(b, dtype=torch.float32, device=dev) if td_out is None else td_out
        loss = torch.empty((), dtype=torch.float32, device=dev) if loss_out is None \
            else loss_out
        nparts = int(L.tsrl_dqn_num_partials(b))
        partials = torch.empty(nparts, dtype=torch.float64, device=dev) if nparts > 1 else None
        _C.check(L.tsrl_dqn_td_fwd_bwd(
            _C.ptr(x), _C.ptr(act, torch.int64), _C.ptr(returns, torch.float32),
            _C.ptr(weight, torch.float32), b, A, int(bool(huber)), _C.ptr(grad_q), _C.ptr(td),
            _C.ptr(partials), _C.ptr(loss), _C.stream_ptr(dev)), "tsrl_dqn_td_fwd_bwd")
        ctx.save_for_backward(grad_q)
        ctx.q_dtype = q.dtype
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(td)
        return loss.clone() if loss_out is not None else loss, td

    @staticmethod
    def backward(ctx, g_loss, g_td):
        (grad_q,) = ctx.saved_tensors
        if g_loss is None:
            return None, None
        if _is_unit_seed(g_loss):  # loss.backward(UNIT): the kernel's gradient as it is
            return grad_q.to(ctx.q_dtype), None
        return (grad_q * g_loss).to(ctx.q_dtype), None


class DQNPolicy(BasePolicy):
    """Constructor arguments, defaults and assertions as the reference's (dqn.py:41-69).

    Attributes that select the device paths: ``fused`` (False: the reference's torch
    formulation throughout), ``fused_adam`` (False: keep ``optim.step()`` even for a plain
    Adam / RMSprop) and ``graph_learn`` (None / True / False, read as on A2CPolicy /
    PPOPolicy: None replays updates of fewer than GRAPH_LEARN_MAX_ROWS rows)."""

    def __init__(self, model: torch.nn.Module, optim: torch.optim.Optimizer,
                 discount_factor: float = 0.99, estimation_step: int = 1,
                 target_update_freq: int = 0, reward_normalization: bool = False,
                 is_double: bool = True, clip_loss_grad: bool = False, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        self.model = model
        self.optim = optim
        self.eps = 0.0
        assert 0.0 <= discount_factor <= 1.0, "discount factor should be in [0, 1]"
        self._gamma = discount_factor
        assert estimation_step > 0, "estimation_step should be greater than 0"
        self._n_step = estimation_step
        self._target = target_update_freq > 0
        self._freq = target_update_freq
        self._iter = 0
        if self._target:
            self.model_old = deepcopy(self.model)
            self.model_old.eval()
        self._rew_norm = reward_normalization
        self._is_double = is_double
        self._clip_loss_grad = clip_loss_grad
        self.fused = True
        self.fused_adam = True
        self.graph_learn = None
        self._graph_failed = False
        self._learn_graphs: Dict[Any, dict] = {}
        self._flat: Optional[FlatAdam] = None
        self._old_flat: Optional[torch.Tensor] = None
        self._old_src: Optional[torch.Tensor] = None  # the flat_param _old_flat mirrors
        self._warm = False

    def set_eps(self, eps: float) -> None:
        self.eps = eps

    def train(self, mode: bool = True) -> "DQNPolicy":
        """dqn.py:75-79: the target network stays in eval mode."""
        self.training = mode
        self.model.train(mode)
        return self

    # -- flat parameter storage -----------------------------------------------------------------
    def _on_device(self) -> bool:
        p = next(self.model.parameters(), None)
        return p is not None and p.is_cuda

    def _fused_learn(self) -> bool:
        """learn() runs the fused loss and the flat optimiser pass; False: the torch
        formulation (``_learn_torch``), as with ``fused = False``."""
        return self.fused and self._on_device()

    def _flat_adam(self) -> Optional[FlatAdam]:
        """The flat gradient / optimiser storage of the Q-network when the optimiser is a plain
        Adam or RMSprop over exactly its parameters (None otherwise: torch's step runs).  The
        target network's parameters then become views into a second flat buffer laid out as
        the first (flat_learn.mirror_target)."""
        if not (self.fused_adam and self._fused_learn()):
            return None
        fa = self._flat
        if fa is None:
            fa = self._flat = FlatAdam(self.model.parameters())
        if not fa.bind_adam(self.optim):
            self._old_flat = None
            return None
        if self._target and not self._old_is_flat(fa):
            self._old_src = fa.flat_param
            self._old_flat = mirror_target(self.model_old, fa.params, self._old_src)
        return fa

    def _old_is_flat(self, fa: FlatAdam) -> bool:
        return target_mirrored(self.model_old, self._old_flat, self._old_src, fa.flat_param)

    def sync_weight(self) -> None:
        """dqn.py:81-83.  With the flat storage bound and no module buffers (BatchNorm
        statistics and the like) the hard sync is one copy between the two flat buffers."""
        fa = self._flat
        if fa is not None and fa.adam_bound(self.optim) and self._old_is_flat(fa) and \
                next(self.model.buffers(), None) is None:
            self._old_flat.copy_(fa.flat_param)
            return
        self.model_old.load_state_dict(self.model.state_dict())

    # -- acting ---------------------------------------------------------------------------------
    def compute_q_value(self, logits: torch.Tensor, mask) -> torch.Tensor:
        """dqn.py:112-120: masked actions pushed below logits.min()."""
        if mask is not None:
            min_value = logits.min() - logits.max() - 1.0
            inv = 1 - torch.as_tensor(np.asarray(mask) if not isinstance(mask, torch.Tensor)
                                      else mask, device=logits.device).to(logits.dtype)
            logits = logits + inv * min_value
        return logits

    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                model: str = "model", input: str = "obs", **kwargs: Any) -> Batch:
        """dqn.py:122-165.  ``act`` is a device int64 tensor (what this package's Collector
        carries), ``logits`` the raw network output; ``obs.mask`` masks actions as in the
        reference."""
        net = getattr(self, model)
        obs = batch[input]
        masked = isinstance(obs, Batch) and "obs" in obs
        logits, hidden = net(obs.obs if masked else obs, state=state,
                             info=batch.get("info", Batch()))
        mask = obs.get("mask") if isinstance(obs, Batch) else None
        if not hasattr(self, "max_action_num"):
            self.max_action_num = logits.shape[1]
        if mask is None:
            act = self._greedy_act(logits)
        else:
            act = self.compute_q_value(logits, mask).max(dim=1)[1]
        return Batch(logits=logits, act=act, state=hidden)

    def _greedy_act(self, logits: torch.Tensor) -> torch.Tensor:
        """The unmasked greedy action of forward() (dqn.py:160-162 with mask None)."""
        return logits.argmax(dim=1)

    def exploration_noise(self, act, batch: Batch):
        """dqn.py:190-203.  The two draws come from NumPy's global stream in the reference's
        order and shapes, so a seeded run consumes it as the reference does; a device ``act``
        is overwritten in place by tsrl_eps_greedy, a NumPy ``act`` on the host."""
        if not isinstance(act, (np.ndarray, torch.Tensor)) or np.isclose(self.eps, 0.0):
            return act
        bsz = len(act)
        u_row = np.random.rand(bsz)
        u_act = np.random.rand(bsz, self.max_action_num)
        obs = batch.obs
        mask = obs.get("mask") if isinstance(obs, Batch) else None
        if isinstance(mask, torch.Tensor) and not (isinstance(act, torch.Tensor) and act.is_cuda):
            mask = mask.cpu().numpy()
        if isinstance(act, np.ndarray) or not act.is_cuda:
            if mask is not None:
                u_act += mask
            rand_act, rows = u_act.argmax(axis=1), u_row < self.eps
            if isinstance(act, np.ndarray):
                act[rows] = rand_act[rows]
            else:
                rows = torch.as_tensor(rows)
                act[rows] = torch.as_tensor(rand_act)[rows].to(act.dtype)
            return act
        dev = act.device
        out = act if act.dtype == torch.int64 and act.is_contiguous() else \
            act.to(torch.int64).contiguous()
        if mask is not None:
            mask = torch.as_tensor(np.asarray(mask) if not isinstance(mask, torch.Tensor)
                                   else mask, device=dev).to(torch.uint8) \
                .reshape(bsz, self.max_action_num).contiguous()
        u_row_d, u_act_d = torch.as_tensor(u_row, device=dev), torch.as_tensor(u_act, device=dev)
        _C.check(_C.lib().tsrl_eps_greedy(
            _C.ptr(out), _C.ptr(u_row_d), _C.ptr(u_act_d), _C.ptr(mask), float(self.eps), bsz,
            int(self.max_action_num), _C.stream_ptr(dev)), "tsrl_eps_greedy")
        if out is not act:
            act.copy_(out)
        return act

    # -- process_fn -----------------------------------------------------------------------------
    def _target_q(self, buffer, indices: np.ndarray) -> torch.Tensor:
        """dqn.py:85-96: Q_target(s_{t+n}, argmax Q_online(s_{t+n}, .)) (double) or
        max Q_target(s_{t+n}, .), for the buffer rows ``indices``.  Only obs_next is gathered;
        the bootstrap value after the forwards is one tsrl_dqn_target_q launch."""
        obs_next = buffer.get(indices, "obs_next") if getattr(buffer, "_save_obs_next", True) \
            else buffer[indices].obs_next
        batch = Batch(obs_next=obs_next, info=Batch())
        masked = isinstance(obs_next, Batch) and "mask" in obs_next
        with torch.no_grad():
            result = self(batch, input="obs_next")
            target_q = self(batch, model="model_old", input="obs_next").logits \
                if self._target else result.logits
        if self.fused and not masked and target_q.is_cuda and target_q.dim() == 2:
            return target_q_device(result.logits if self._is_double else None, target_q,
                                   self._is_double)
        if self._is_double:
            return target_q[torch.arange(len(result.act), device=target_q.device), result.act]
        return target_q.max(dim=1)[0]

    def process_fn(self, batch: Batch, buffer, indices: np.ndarray) -> Batch:
        """dqn.py:98-110: n-step returns over the buffer (tsrl_nstep_return)."""
        return self.compute_nstep_return(batch, buffer, indices, self._target_q, self._gamma,
                                         self._n_step, self._rew_norm)

    # -- learn ----------------------------------------------------------------------------------
    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        """dqn.py:167-188.  ``batch.weight`` leaves as the detached device TD error (what a
        prioritized buffer's update_weight takes); the loss is the update's one host read."""
        fa = self._flat_adam()
        if self._target and self._iter % self._freq == 0:
            self.sync_weight()
        weight = batch.pop("weight", None)
        obs = batch.obs
        net_in = obs.obs if isinstance(obs, Batch) and "obs" in obs else obs
        if not self._fused_learn():
            loss, td = self._learn_torch(batch, weight)
        else:
            dev = next(self.model.parameters()).device
            n = len(batch.returns)
            act = self._learn_act(batch, dev, n)
            returns = self._returns_rows(batch, dev, n)
            w = self._loss_weight(weight, dev, n)
            extra = self._learn_inputs(batch)
            out = None
            if fa is not None:
                for f in self._flats(fa):
                    f.set_lr()
                if self._warm and net_in is obs and self._graph_ok(net_in, n) and \
                        all(isinstance(e, torch.Tensor) and e.is_cuda for e in extra):
                    out = self._graph_step(fa, net_in, act, returns, w, *extra)
            if out is None:
                out = self._step(fa, net_in, batch.get("info", Batch()), act, returns, w, *extra)
            loss, td = out
            self._warm = True
        batch.weight = td.detach()  # prio-buffer
        self._iter += 1
        return self._learn_result(loss)

    def _learn_torch(self, batch: Batch, weight):
        """The reference's op sequence as written (dqn.py:170-186), on whatever device the
        network lives on."""
        self.optim.zero_grad()
        q = self(batch).logits
        act = torch.as_tensor(batch.act, device=q.device).reshape(len(q)).long()
        q = q[torch.arange(len(q), device=q.device), act]
        returns = torch.as_tensor(batch.returns, device=q.device).flatten().to(q.dtype)
        td_error = returns - q
        if self._clip_loss_grad:
            loss = torch.nn.functional.huber_loss(q.reshape(-1, 1), returns.reshape(-1, 1),
                                                  reduction="mean")
        else:
            w = 1.0 if weight is None else torch.as_tensor(weight, device=q.device).to(q.dtype)
            loss = (td_error.pow(2) * w).mean()
        loss.backward()
        self.optim.step()
        return loss.detach(), td_error

    # -- what a subclass's update differs in -----------------------------------------------------
    def _learn_inputs(self, batch: Batch) -> tuple:
        """The inputs of one update beyond obs / act / returns / weight (static inputs of the
        learn graph, handed on to ``_before_forward``)."""
        return ()

    def _learn_act(self, batch: Batch, dev, n: int) -> torch.Tensor:
        """The taken actions as a device int64 [n] (BranchingDQNPolicy: [n, K])."""
        return torch.as_tensor(batch.act, device=dev).reshape(n).to(torch.int64).contiguous()

    def _returns_rows(self, batch: Batch, dev, n: int) -> torch.Tensor:
        return f32_rows(batch.returns, dev, n)

    def _flats(self, fa: FlatAdam) -> tuple:
        """Every flat optimiser storage one update steps (FQFPolicy adds its proposal
        network's)."""
        return (fa,)

    def _loss_out(self, dev) -> torch.Tensor:
        """The static loss output of a learn graph (FQFPolicy's holds its four scalars)."""
        return torch.empty((), dtype=torch.float32, device=dev)

    def _learn_result(self, loss: torch.Tensor) -> Dict[str, float]:
        """learn()'s dictionary from the device loss: the update's one host read."""
        return {"loss": loss.item()}

    def _loss_weight(self, weight, dev, n: int) -> Optional[torch.Tensor]:
        return None if weight is None or self._clip_loss_grad else f32_rows(weight, dev, n)

    def _before_forward(self, info, *extra):
        """No-grad work on the extra inputs ahead of the forward on obs; its result reaches
        ``_fused_loss``."""
        return None

    def _forward_q(self, obs, info, aux):
        """The online network's output at obs and what ``_fused_loss`` gets as ``aux``
        (IQNPolicy hands fractions in and takes them back)."""
        return self.model(obs, state=None, info=info)[0], aux

    def _fused_loss(self, q, act, returns, weight, aux, td_out, loss_out):
        """(loss, per-row vector that leaves as batch.weight) of the network output q."""
        return _DQNLoss.apply(q, (act, returns, weight, self._clip_loss_grad, td_out, loss_out))

    def _step(self, fa: Optional[FlatAdam], obs, info, act, returns, weight, *extra,
              td_out=None, loss_out=None):
        """Forward, fused TD loss, backward, optimiser step; returns (loss, td_error)."""
        aux = self._before_forward(info, *extra)
        q, aux = self._forward_q(obs, info, aux)
        loss, td = self._fused_loss(q, act, returns, weight, aux, td_out, loss_out)
        if fa is None:
            self.optim.zero_grad()
            loss.backward()
            self.optim.step()
            return loss.detach(), td
        with flat_backward((fa,)):
            loss.backward(_unit_seed(loss.device))
        fa.clip_adam(None)  # the reference clips nothing: one optimiser pass
        return loss.detach(), td

    # -- HIP-graph replay of one update ----------------------------------------------------------
    def _graph_ok(self, obs, n: int) -> bool:
        """Unmasked device observations, no earlier capture failure, and -- as in
        FusedLearnMixin._learn_cat -- conv trunks only with graph_learn=True."""
        if self._graph_failed or not isinstance(obs, torch.Tensor) or not obs.is_cuda:
            return False
        return self._use_graph(n) and (obs.dim() == 2 or self.graph_learn is True)

    def _capture(self, graph):
        """The capture context of a learn graph (utils.capture.graph_capture)."""
        return graph_capture(graph)

    def _graph_addrs(self) -> tuple:
        """Further addresses a subclass's captured update is tied to."""
        return ()

    def _graph_step(self, fa: FlatAdam, obs, act, returns, weight, *extra):
        """One update's forward, loss, backward and flat optimiser pass replayed from a HIP
        graph captured once per (batch size, observation shape and dtype, flat addresses);
        static copies of obs / act / returns / weight (and a subclass's extra inputs) feed it,
        the loss and the TD errors come out of static outputs (flat_learn.replay_learn_graph).
        None if the capture failed (this and every later update then run eagerly)."""
        addr = ()
        for f in self._flats(fa):
            f.bind_grads()
            addr += (f.flat_grad.data_ptr(), tuple(p.data_ptr() for p in f.params))
        addr += self._graph_addrs()
        key = (len(act), tuple(obs.shape), obs.dtype, weight is not None,
               tuple((tuple(e.shape), e.dtype) for e in extra))
        out = replay_learn_graph(
            self._learn_graphs, key, addr, (obs, act, returns, weight, *extra),
            lambda: (torch.empty(len(act), dtype=torch.float32, device=act.device),
                     self._loss_out(act.device)),
            lambda s, td, loss: self._step(fa, s[0], Batch(), *s[1:], td_out=td, loss_out=loss),
            self._capture)
        if out is None:
            self._graph_failed = True
        return out
