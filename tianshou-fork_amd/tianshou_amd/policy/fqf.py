"""FQFPolicy (tianshou/policy/modelfree/fqf.py:12-177): fully parameterized quantile function,
arXiv:1911.02140, on QRDQNPolicy's device path.

FQF is IQN whose fractions come from a proposal network (utils/net.py
``FractionProposalNetwork``) trained by a loss of its own; the quantile network (utils/net.py
``FullQuantileFunction``) returns ((quantiles, fractions, quantiles_tau), hidden).  The proposal
forward is one tsrl_fqf_propose_fwd launch, acting and ``_target_q`` are tsrl_fqf_select (the
weighted sum over the proposed intervals, the greedy action, the target network's row), the
quantile Huber loss is tsrl_iqn_loss_fwd_bwd at tau_hats and the fraction loss with its
backward to the proposal logits is tsrl_fqf_fraction_loss_fwd_bwd.  The fraction loss reaches
only the proposal network and the quantile loss only the quantile network, so one backward call
serves both and each network has a flat optimiser pass of its own; an update has no random
input, so all of it -- both forwards, both losses, both backwards, both optimiser passes --
replays from one HIP graph.  The four scalars leave in one device vector with one host read.

``_target_q`` skips the reference's quantiles_tau pass at obs_next, whose result nobody reads.
A ``model`` that is not this package's FullQuantileFunction or a ``fraction_model`` that is not
its FractionProposalNetwork is never captured; it still gets the fused losses from what it
returned (the fraction loss then hands the gradients of taus and entropies to autograd).
``fused = False`` runs the reference's op sequence on torch, the proposal and the cosine
embedding included; so does learn() with more fractions than the kernels take
(``_C.DIST_MAX_N``).  ``fused = True`` is the default: in tools/fqf_update_bench.py
(profiles/fqf_update_bench.log) the graph leg takes 1.47-1.48 ms against the torch leg's
3.97-4.51 ms on the MLP config and 1.66-1.67 against 3.92-3.94 ms on the Atari config, more than
the torch leg's run-to-run spread in both.
"""
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.dqn import DQNPolicy
from tianshou_amd.policy.dqn_dist import _rows
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import flat_backward
from tianshou_amd.policy.iqn import _IQNLoss, _dptr, _strided
from tianshou_amd.policy.onpolicy import _is_unit_seed, _unit_seed
from tianshou_amd.policy.qrdqn import QRDQNPolicy
from tianshou_amd.utils.net import (FractionProposalNetwork, FullQuantileFunction,
                                    ImplicitQuantileNetwork)


def fqf_select(sel: torch.Tensor, taus: torch.Tensor, eval_: Optional[torch.Tensor] = None,
               want_q: bool = False, want_act: bool = True, want_row: bool = False
               ) -> Tuple[Optional[torch.Tensor], ...]:
    """(q [b, A], act [b] int64, row [b, N]) of ``sel`` [b, A, N], in either layout, at the
    fractions ``taus`` [b, N + 1]; an output not asked for is None.  q = ((taus[:, 1:] -
    taus[:, :-1]).unsqueeze(1) * sel).sum(2) (fqf.py:103-107); act = its first argmax; row =
    (eval_ if given else sel)[r, act[r], :]."""
    sel, sa, sn = _strided(sel)
    b, A, N = sel.shape
    dev = sel.device
    taus = taus.detach().float().contiguous()
    _rows(taus, b, N + 1, "fqf_select taus")
    ea, em, ev_ptr = 0, 0, None
    if eval_ is not None:
        eval_, ea, em = _strided(eval_)
        if eval_.shape != sel.shape:
            raise ValueError(f"fqf_select: eval {tuple(eval_.shape)} against sel {(b, A, N)}")
        ev_ptr = _dptr(eval_)
    q = torch.empty(b, A, dtype=torch.float32, device=dev) if want_q else None
    act = torch.empty(b, dtype=torch.int64, device=dev) if want_act else None
    row = torch.empty(b, N, dtype=torch.float32, device=dev) if want_row else None
    _C.check(_C.lib().tsrl_fqf_select(_dptr(sel), sa, sn, ev_ptr, ea, em, _dptr(taus), b, A, N,
                                      _C.ptr(q), _C.ptr(act), _C.ptr(row), _C.stream_ptr(dev)),
             "tsrl_fqf_select")
    return q, act, row


def fraction_loss_kernel(curr, qtau, act, taus, logp, entropies, ent_coef: float,
                         losses: Optional[torch.Tensor] = None, want_grad_taus: bool = False):
    """One tsrl_fqf_fraction_loss_fwd_bwd launch: (losses [2] = (fraction loss, entropy loss),
    g_logits [b, N], gradient_of_taus [b, N - 1] or None).  curr [b, A, N] and qtau [b, A, N - 1]
    are read in place in either layout; ``losses`` (optional) receives the two scalars."""
    x, sa, sn = _strided(curr)
    b, A, N = x.shape
    qt, ta, tn = _strided(qtau)
    if qt.shape != (b, A, N - 1):
        raise ValueError(f"fraction loss: quantiles_tau {tuple(qt.shape)} against {(b, A, N)}")
    dev = x.device
    taus, logp = taus.detach().float().contiguous(), logp.detach().float().contiguous()
    entropies = entropies.detach().float().contiguous()
    _rows(act, b, 1, "fraction loss act", torch.int64)
    _rows(taus, b, N + 1, "fraction loss taus")
    _rows(logp, b, N, "fraction loss logp")
    _rows(entropies, b, 1, "fraction loss entropies")
    _rows(losses, 1, 2, "fraction loss losses")
    g_logits = torch.empty(b, N, dtype=torch.float32, device=dev)
    g_taus = torch.empty(b, N - 1, dtype=torch.float32, device=dev) if want_grad_taus else None
    if losses is None:
        losses = torch.empty(2, dtype=torch.float32, device=dev)
    partials = torch.empty(2 * b, dtype=torch.float64, device=dev) if b > 1 else None
    _C.check(_C.lib().tsrl_fqf_fraction_loss_fwd_bwd(
        _dptr(x), sa, sn, _dptr(qt), ta, tn, _C.ptr(act), _dptr(taus), _dptr(logp),
        _dptr(entropies), float(ent_coef), b, A, N, _dptr(g_logits), _C.ptr(g_taus),
        _C.ptr(partials), _dptr(losses), _C.stream_ptr(dev)), "tsrl_fqf_fraction_loss_fwd_bwd")
    return losses, g_logits, g_taus


class _FQFFractionLoss(torch.autograd.Function):
    """fqf.py:142-164 as tsrl_fqf_fraction_loss_fwd_bwd: returns (fraction_loss - ent_coef *
    entropy_loss, losses [2]).  With ``logits`` (the proposal network's, whose softmax gave taus,
    logp and entropies) the backward hands back the kernel's g_logits; with ``logits`` None the
    fractions came from a foreign network, and taus and entropies get gradient_of_taus / b and
    -ent_coef / b.  ctx_args: (curr [b, A, N], quantiles_tau [b, A, N - 1], act [b], logp [b, N]
    or None, ent_coef, out [4] or None); ``out``, the static output of a captured graph, receives
    (., fraction loss, entropy loss, the returned scalar)."""

    @staticmethod
    def forward(ctx, logits, taus, entropies, ctx_args):
        curr, qtau, act, logp, ent_coef, out = ctx_args
        foreign = logits is None
        if foreign:  # the p_k the foreign network's taus imply
            t = taus.detach().float()
            logp = (t[:, 1:] - t[:, :-1]).log()
        losses, g_logits, g_taus = fraction_loss_kernel(
            curr, qtau, act, taus, logp, entropies, ent_coef,
            None if out is None else out[1:3], want_grad_taus=foreign)
        if out is None:
            handle = torch.sub(losses[0], losses[1], alpha=float(ent_coef))
        else:
            torch.sub(losses[0], losses[1], alpha=float(ent_coef), out=out[3])
            handle = out[3].clone()
        ctx.foreign, ctx.ent_coef, ctx.b = foreign, float(ent_coef), taus.shape[0]
        ctx.save_for_backward(g_taus if foreign else g_logits)
        ctx.dtypes = (None if foreign else logits.dtype, taus.dtype, entropies.dtype)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(losses)
        return handle, losses

    @staticmethod
    def backward(ctx, g, g_losses):
        (grad,) = ctx.saved_tensors
        if g is None:
            return None, None, None, None
        if ctx.foreign:
            g_taus = F.pad(grad, (1, 1)) * (g / ctx.b)
            g_ent = (g * (-ctx.ent_coef / ctx.b)).expand(ctx.b)
            return None, g_taus.to(ctx.dtypes[1]), g_ent.to(ctx.dtypes[2]), None
        if not _is_unit_seed(g):  # backward(UNIT): the kernel's gradient as it is
            grad = grad * g
        return grad.to(ctx.dtypes[0]), None, None, None


class FQFPolicy(QRDQNPolicy):
    """Constructor arguments, defaults and attributes as the reference's (fqf.py:39-59)."""

    @property
    def fused(self) -> bool:
        return self._fused

    @fused.setter
    def fused(self, value: bool) -> None:
        """As IQNPolicy's: False also sends both networks' cosine embedding and the proposal
        network to the torch lines, so that leg is the reference's op sequence throughout."""
        object.__setattr__(self, "_fused", bool(value))
        for net in (getattr(self, "model", None), getattr(self, "model_old", None)):
            for m in net.modules() if net is not None else ():
                if isinstance(m, ImplicitQuantileNetwork):
                    m.fused_embed = bool(value)
        if isinstance(getattr(self, "propose_model", None), FractionProposalNetwork):
            self.propose_model.fused = bool(value)

    def __init__(self, model: torch.nn.Module, optim: torch.optim.Optimizer,
                 fraction_model: torch.nn.Module, fraction_optim: torch.optim.Optimizer,
                 discount_factor: float = 0.99, num_fractions: int = 32, ent_coef: float = 0.0,
                 estimation_step: int = 1, target_update_freq: int = 0,
                 reward_normalization: bool = False, **kwargs: Any) -> None:
        super().__init__(model, optim, discount_factor, num_fractions, estimation_step,
                         target_update_freq, reward_normalization, **kwargs)
        self.propose_model = fraction_model
        self._ent_coef = ent_coef
        self._fraction_optim = fraction_optim
        self._frac_flat: Optional[FlatAdam] = None
        self.fused = self._fused  # hand the switch to the proposal network as well

    def _own_nets(self) -> bool:
        return isinstance(self.model, FullQuantileFunction) and \
            isinstance(self.propose_model, FractionProposalNetwork)

    # -- flat storage: one per network -----------------------------------------------------------
    def _flat_adam(self) -> Optional[FlatAdam]:
        """The quantile network's flat storage, and the proposal network's beside it; None
        (torch's step for both) unless both optimisers are a plain Adam or RMSprop."""
        fa = super()._flat_adam()
        if fa is None or next(self.propose_model.parameters(), None) is None:
            return None
        ff = self._frac_flat
        if ff is None:
            ff = self._frac_flat = FlatAdam(self.propose_model.parameters())
        return fa if ff.bind_adam(self._fraction_optim) else None

    def _flats(self, fa: FlatAdam) -> tuple:
        return (fa, self._frac_flat)

    # -- acting ---------------------------------------------------------------------------------
    def _weighted_q(self, logits: torch.Tensor, taus: torch.Tensor, mask) -> torch.Tensor:
        """fqf.py:103-107."""
        weighted_logits = (taus[:, 1:] - taus[:, :-1]).unsqueeze(1) * logits
        return DQNPolicy.compute_q_value(self, weighted_logits.sum(2), mask)

    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                model: str = "model", input: str = "obs", fractions: Optional[Batch] = None,
                **kwargs: Any) -> Batch:
        """fqf.py:76-117; ``act`` is a device int64 tensor as in DQNPolicy.forward."""
        net = getattr(self, model)
        obs = batch[input]
        masked = isinstance(obs, Batch) and "obs" in obs
        kw = dict(propose_model=self.propose_model, state=state, info=batch.get("info", Batch()))
        if fractions is not None:
            kw["fractions"] = fractions
        if "want_quantiles_tau" in kwargs and isinstance(net, FullQuantileFunction):
            kw["want_quantiles_tau"] = kwargs["want_quantiles_tau"]
        (logits, proposed, quantiles_tau), hidden = net(obs.obs if masked else obs, **kw)
        if fractions is None:
            fractions = proposed
        mask = obs.get("mask") if isinstance(obs, Batch) else None
        if not hasattr(self, "max_action_num"):
            self.max_action_num = logits.shape[1]
        if mask is None and self.fused and logits.is_cuda and logits.dim() == 3:
            act = fqf_select(logits, fractions.taus)[1]
        else:
            act = self._weighted_q(logits, fractions.taus, mask).max(dim=1)[1]
        return Batch(logits=logits, act=act, state=hidden, fractions=fractions,
                     quantiles_tau=quantiles_tau)

    def _next_rows(self, batch: Batch) -> torch.Tensor:
        """fqf.py:61-74: the target network's quantiles, at the online network's fractions, of
        the online network's greedy action at batch.obs_next -- one no-grad forward per network,
        neither with the quantiles_tau pass, and one tsrl_fqf_select launch; masked observations
        and the torch leg go through forward()."""
        obs_next = batch.obs_next
        masked = isinstance(obs_next, Batch) and "mask" in obs_next
        with torch.no_grad():
            if self.fused and not masked and self._on_device():
                net_in = obs_next.obs if isinstance(obs_next, Batch) and "obs" in obs_next \
                    else obs_next
                kw = dict(propose_model=self.propose_model, state=None,
                          info=batch.get("info", Batch()))
                skip = dict(want_quantiles_tau=False) if self._own_nets() else {}
                (sel, fractions, _), _ = self.model(net_in, **kw, **skip)
                if not hasattr(self, "max_action_num"):
                    self.max_action_num = sel.shape[1]
                ev = self.model_old(net_in, fractions=fractions, **kw, **skip)[0][0] \
                    if self._target else None
                return fqf_select(sel, fractions.taus, ev, want_act=False, want_row=True)[2]
            result = self(batch, input="obs_next", want_quantiles_tau=False)
            act, next_dist = result.act, result.logits
            if self._target:
                next_dist = self(batch, model="model_old", input="obs_next",
                                 fractions=result.fractions, want_quantiles_tau=False).logits
            return next_dist[torch.arange(len(act), device=next_dist.device), act, :]

    # -- learn (fqf.py:119-177): DQNPolicy.learn with these hooks --------------------------------
    def _graph_ok(self, obs, n: int) -> bool:
        """Foreign networks are never captured."""
        return self._own_nets() and super()._graph_ok(obs, n)

    def _loss_out(self, dev) -> torch.Tensor:
        """(quantile loss, fraction loss, entropy loss, fraction - ent_coef * entropy)."""
        return torch.empty(4, dtype=torch.float32, device=dev)

    def _learn_result(self, loss: torch.Tensor) -> Dict[str, float]:
        quantile, fraction, entropy, fraction_entropy = loss.tolist()
        return {"loss": quantile + fraction_entropy, "loss/quantile": quantile,
                "loss/fraction": fraction, "loss/entropy": entropy}

    def _forward_parts(self, obs, info):
        """(proposal logits or None, taus, tau_hats, entropies, logp or None, quantiles [b, A,
        N], quantiles_tau [b, A, N - 1]) of one training forward at obs.  This package's networks
        on the kernel path are walked here, so that the proposal's by-products reach the
        fraction loss; anything else is called as fqf.py:123 calls it."""
        model, propose = self.model, self.propose_model
        if self._own_nets():
            h, _ = model.preprocess(obs, state=None)
            if propose.takes_kernel(h):
                logits, taus, tau_hats, entropies, logp = propose.propose(h.detach())
                quantiles = model._compute_quantiles(h, tau_hats)
                with torch.no_grad():
                    quantiles_tau = model._compute_quantiles(h, taus[:, 1:-1])
                return logits, taus, tau_hats, entropies, logp, quantiles, quantiles_tau
        (quantiles, fr, quantiles_tau), _ = model(obs, propose_model=propose, state=None,
                                                  info=info)
        if quantiles_tau is None:  # discrete.py:313: computed only while training
            raise RuntimeError("FQFPolicy.learn needs quantiles_tau: call policy.train() first")
        return None, fr.taus, fr.tau_hats, fr.entropies, None, quantiles, quantiles_tau

    def _step(self, fa: Optional[FlatAdam], obs, info, act, returns, weight, *extra,
              td_out=None, loss_out=None):
        """Both forwards, both fused losses, both backwards, both optimiser steps; returns (the
        four scalars as a device vector, the priorities)."""
        logits, taus, tau_hats, entropies, logp, quantiles, quantiles_tau = \
            self._forward_parts(obs, info)
        out = self._loss_out(quantiles.device) if loss_out is None else loss_out
        quantile_loss, prio = _IQNLoss.apply(
            quantiles, (act, returns, tau_hats.detach().float().contiguous(), weight, td_out,
                        out[0]))
        fraction_entropy_loss, _ = _FQFFractionLoss.apply(
            logits, taus.detach() if logits is not None else taus, entropies,
            (quantiles, quantiles_tau, act, logp, self._ent_coef, out))
        if fa is None:
            self._fraction_optim.zero_grad()
            fraction_entropy_loss.backward(retain_graph=True)
            self._fraction_optim.step()
            self.optim.zero_grad()
            quantile_loss.backward()
            self.optim.step()
            return out.detach(), prio
        unit = _unit_seed(out.device)
        with flat_backward(self._flats(fa)):
            torch.autograd.backward((fraction_entropy_loss, quantile_loss), (unit, unit))
        self._frac_flat.clip_adam(None)
        fa.clip_adam(None)  # the reference clips nothing: one optimiser pass per network
        return out.detach(), prio

    def _learn_torch(self, batch: Batch, weight):
        """The reference's op sequence as written (fqf.py:123-170); returns the four scalars as
        one vector and the priorities that leave as ``batch.weight``."""
        out = self(batch)
        curr_dist_orig = out.logits
        taus, tau_hats = out.fractions.taus, out.fractions.tau_hats
        n = len(curr_dist_orig)
        dev = curr_dist_orig.device
        rows = torch.arange(n, device=dev)
        act = torch.as_tensor(batch.act, device=dev).reshape(n).long()
        curr_dist = curr_dist_orig[rows, act, :].unsqueeze(2)
        target_dist = torch.as_tensor(batch.returns, device=dev).unsqueeze(1)
        dist_diff = F.smooth_l1_loss(target_dist, curr_dist, reduction="none")
        huber_loss = (dist_diff * (tau_hats.unsqueeze(2) - (target_dist - curr_dist).detach()
                                   .le(0.).float()).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else torch.as_tensor(weight, device=dev).to(curr_dist.dtype)
        quantile_loss = (huber_loss * w).mean()
        prio = dist_diff.detach().abs().sum(-1).mean(1)
        with torch.no_grad():
            sa_quantile_hats = curr_dist_orig[rows, act, :]
            sa_quantiles = out.quantiles_tau[rows, act, :]
            values_1 = sa_quantiles - sa_quantile_hats[:, :-1]
            signs_1 = sa_quantiles > torch.cat(
                [sa_quantile_hats[:, :1], sa_quantiles[:, :-1]], dim=1)
            values_2 = sa_quantiles - sa_quantile_hats[:, 1:]
            signs_2 = sa_quantiles < torch.cat(
                [sa_quantiles[:, 1:], sa_quantile_hats[:, -1:]], dim=1)
            gradient_of_taus = torch.where(signs_1, values_1, -values_1) + \
                torch.where(signs_2, values_2, -values_2)
        fraction_loss = (gradient_of_taus * taus[:, 1:-1]).sum(1).mean()
        entropy_loss = out.fractions.entropies.mean()
        fraction_entropy_loss = fraction_loss - self._ent_coef * entropy_loss
        self._fraction_optim.zero_grad()
        fraction_entropy_loss.backward(retain_graph=True)
        self._fraction_optim.step()
        self.optim.zero_grad()
        quantile_loss.backward()
        self.optim.step()
        return torch.stack((quantile_loss.detach(), fraction_loss.detach(),
                            entropy_loss.detach(), fraction_entropy_loss.detach())), prio
