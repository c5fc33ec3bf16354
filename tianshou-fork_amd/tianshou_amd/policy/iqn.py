"""IQNPolicy (tianshou/policy/modelfree/iqn.py:11-112): implicit quantile networks,
arXiv:1806.06923, on QRDQNPolicy's device path.

The network (utils/net.py ``ImplicitQuantileNetwork``) returns ((out, taus), hidden): N quantile
values per action at N fractions drawn per row, ``out`` the [b, A, N] view of the head's
quantile-major [b, N, A] output.  Acting and ``_target_q`` are tsrl_iqn_select (the mean over
the quantiles, the greedy action, the target network's row of M quantiles) and learn() is
tsrl_iqn_loss_fwd_bwd (the N x M pairs of a row against that row's own fractions); both read
the view in place through its strides, and the loss hands its gradient back in the same layout.

Every fraction the policy draws comes from ``_sample_taus`` and reaches the network as
``taus=``, in the reference's order within an update: the online network at obs_next, the target
network at obs_next (when there is one), the online network at obs.  The last draw is made ahead
of the learn graph (``_learn_inputs``), so the captured update holds no random node.  A model
that is not this package's ImplicitQuantileNetwork draws inside its own forward: it is never
handed ``taus=`` and never captured, and still gets the fused loss with the fractions it
returned.  ``fused = False`` runs the reference's op sequence on torch, the networks' cosine
embedding included (the setter hands the value to ``ImplicitQuantileNetwork.fused_embed``); so
does learn() with more fractions than the loss kernel takes (``_C.DIST_MAX_N``).  ``fused =
True`` is the default: in tools/iqn_update_bench.py (profiles/iqn_update_bench.log) the graph
leg takes 1.29-1.30 ms against the torch leg's 2.75-3.13 ms on the MLP config and 1.42-1.43
against 2.84-3.02 ms on the Atari config, more than the torch leg's run-to-run spread in both.
"""
from typing import Any, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.dqn_dist import _rows
from tianshou_amd.policy.onpolicy import _is_unit_seed
from tianshou_amd.policy.qrdqn import QRDQNPolicy
from tianshou_amd.utils.net import ImplicitQuantileNetwork


def _strided(t: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    """(x, sA, sN): ``t`` [b, A, N] as f32 device memory one of the kernels' two layouts reads in
    place -- contiguous, or the transposed view of a contiguous [b, N, A] -- and the element
    strides of its A and N axes; anything else is copied to contiguous storage."""
    x = t.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.dim() != 3:
        raise ValueError(f"need [b, A, N], got {tuple(x.shape)}")
    A, N = x.shape[1], x.shape[2]
    if x.is_contiguous():
        return x, N, 1
    if x.transpose(1, 2).is_contiguous():
        return x, 1, A
    return x.contiguous(), N, 1


def _dptr(x: torch.Tensor) -> int:
    if x.device.type != "cuda":
        raise _C.TsrlError(f"libtsrl kernels need HIP device tensors; got a tensor on {x.device}")
    return x.data_ptr()


def iqn_select(sel: torch.Tensor, eval_: Optional[torch.Tensor] = None, want_q: bool = False,
               want_act: bool = True, want_row: bool = False
               ) -> Tuple[Optional[torch.Tensor], ...]:
    """(q [b, A], act [b] int64, row) of ``sel`` [b, A, N], in either layout; an output not
    asked for is None.  q = sel.mean(2); act = its first argmax; row = eval_[r, act[r], :]
    ([b, M], eval_ being [b, A, M]) or, without eval_, sel's row ([b, N])."""
    sel, sa, sn = _strided(sel)
    b, A, N = sel.shape
    dev = sel.device
    M, ea, em, ev_ptr = N, 0, 0, None
    if eval_ is not None:
        eval_, ea, em = _strided(eval_)
        if eval_.shape[:2] != (b, A):
            raise ValueError(f"iqn_select: eval {tuple(eval_.shape)} against sel {(b, A, N)}")
        M, ev_ptr = eval_.shape[2], _dptr(eval_)
    q = torch.empty(b, A, dtype=torch.float32, device=dev) if want_q else None
    act = torch.empty(b, dtype=torch.int64, device=dev) if want_act else None
    row = torch.empty(b, M, dtype=torch.float32, device=dev) if want_row else None
    _C.check(_C.lib().tsrl_iqn_select(_dptr(sel), sa, sn, ev_ptr, ea, em, b, A, N, M, _C.ptr(q),
                                      _C.ptr(act), _C.ptr(row), _C.stream_ptr(dev)),
             "tsrl_iqn_select")
    return q, act, row


class _IQNLoss(torch.autograd.Function):
    """iqn.py:93-108 as tsrl_iqn_loss_fwd_bwd.  dist is the network's [b, A, N] output, read
    through the strides of the view it is; the gradient goes back in the same layout.
    ctx_args: (act [b], returns [b, M], taus [b, N], weight [b] or None, prio_out, loss_out);
    returns (loss, prio [b])."""

    @staticmethod
    def forward(ctx, dist, ctx_args):
        act, returns, taus, weight, vec_out, loss_out = ctx_args
        x, sa, sn = _strided(dist)
        b, A, N = x.shape
        dev = x.device
        if returns.dim() != 2 or returns.shape[0] != b:
            raise ValueError(f"_IQNLoss: returns {tuple(returns.shape)} for {b} rows")
        M = returns.shape[1]
        _rows(act, b, 1, "_IQNLoss act", torch.int64)
        _rows(returns, b, M, "_IQNLoss returns")
        _rows(taus, b, N, "_IQNLoss taus")
        _rows(weight, b, 1, "_IQNLoss weight")
        _rows(vec_out, b, 1, "_IQNLoss prio_out")
        grad = torch.empty(b, N, A, dtype=torch.float32, device=dev).transpose(1, 2) \
            if (sa, sn) == (1, A) else torch.empty(b, A, N, dtype=torch.float32, device=dev)
        vec = torch.empty(b, dtype=torch.float32, device=dev) if vec_out is None else vec_out
        loss = torch.empty((), dtype=torch.float32, device=dev) if loss_out is None \
            else loss_out
        partials = torch.empty(b, dtype=torch.float64, device=dev) if b > 1 else None
        _C.check(_C.lib().tsrl_iqn_loss_fwd_bwd(
            _dptr(x), sa, sn, _C.ptr(act), _C.ptr(returns), _C.ptr(taus), _C.ptr(weight), b, A,
            N, M, _dptr(grad), _C.ptr(vec), _C.ptr(partials), _C.ptr(loss), _C.stream_ptr(dev)),
            "tsrl_iqn_loss_fwd_bwd")
        ctx.save_for_backward(grad)
        ctx.in_dtype = dist.dtype
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(vec)
        return loss.clone() if loss_out is not None else loss, vec

    @staticmethod
    def backward(ctx, g_loss, g_vec):
        (grad,) = ctx.saved_tensors
        if g_loss is None:
            return None, None
        if _is_unit_seed(g_loss):  # loss.backward(UNIT): the kernel's gradient as it is
            return grad.to(ctx.in_dtype), None
        return (grad * g_loss).to(ctx.in_dtype), None


class IQNPolicy(QRDQNPolicy):
    """Constructor arguments, defaults, assertions and attributes as the reference's
    (iqn.py:38-60)."""

    # acting draws fractions on the host side of the launch: the Collector does not capture it
    eager_collect_step = True

    @property
    def fused(self) -> bool:
        return self._fused

    @fused.setter
    def fused(self, value: bool) -> None:
        """As RainbowPolicy's: False also sends both networks' cosine embedding to the torch
        lines (``ImplicitQuantileNetwork.fused_embed``), so that leg is the reference's op
        sequence throughout."""
        object.__setattr__(self, "_fused", bool(value))
        for net in (getattr(self, "model", None), getattr(self, "model_old", None)):
            for m in net.modules() if net is not None else ():
                if isinstance(m, ImplicitQuantileNetwork):
                    m.fused_embed = bool(value)

    def __init__(self, model: torch.nn.Module, optim: torch.optim.Optimizer,
                 discount_factor: float = 0.99, sample_size: int = 32,
                 online_sample_size: int = 8, target_sample_size: int = 8,
                 estimation_step: int = 1, target_update_freq: int = 0,
                 reward_normalization: bool = False, **kwargs: Any) -> None:
        super().__init__(model, optim, discount_factor, sample_size, estimation_step,
                         target_update_freq, reward_normalization, **kwargs)
        assert sample_size > 1, "sample_size should be greater than 1"
        assert online_sample_size > 1, "online_sample_size should be greater than 1"
        assert target_sample_size > 1, "target_sample_size should be greater than 1"
        self._sample_size = sample_size  # for policy eval
        self._online_sample_size = online_sample_size
        self._target_sample_size = target_sample_size

    # -- fractions ------------------------------------------------------------------------------
    def _sample_taus(self, shape: Tuple[int, int], device) -> torch.Tensor:
        """Every fraction this policy draws: the reference's torch.rand(b, sample_size)
        (discrete.py:208).  A test replaces it with recorded draws."""
        return torch.rand(*shape, dtype=torch.float32, device=device)

    def _own_net(self, net: Optional[torch.nn.Module] = None) -> bool:
        return isinstance(self.model if net is None else net, ImplicitQuantileNetwork)

    def _size_of(self, model: str) -> int:
        """iqn.py:70-75."""
        if model == "model_old":
            return self._target_sample_size
        return self._online_sample_size if self.training else self._sample_size

    def _net_forward(self, model: str, obs, state, info, taus: Optional[torch.Tensor] = None):
        """((out, taus), hidden) of the network ``model`` at ``sample_size`` fractions: this
        package's network gets them from ``_sample_taus`` (or ``taus``), any other draws its
        own."""
        net = getattr(self, model)
        size = self._size_of(model)
        if not self._own_net(net):
            return net(obs, sample_size=size, state=state, info=info)
        if taus is None:
            taus = self._sample_taus((len(obs), size), next(net.parameters()).device)
        return net(obs, sample_size=size, taus=taus, state=state, info=info)

    # -- acting ---------------------------------------------------------------------------------
    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                model: str = "model", input: str = "obs", **kwargs: Any) -> Batch:
        """iqn.py:62-86; ``act`` is a device int64 tensor as in DQNPolicy.forward."""
        obs = batch[input]
        masked = isinstance(obs, Batch) and "obs" in obs
        (logits, taus), hidden = self._net_forward(model, obs.obs if masked else obs, state,
                                                   batch.get("info", Batch()))
        mask = obs.get("mask") if isinstance(obs, Batch) else None
        if not hasattr(self, "max_action_num"):
            self.max_action_num = logits.shape[1]
        if mask is None:
            act = self._greedy_act(logits)
        else:
            act = self.compute_q_value(logits, mask).max(dim=1)[1]
        return Batch(logits=logits, act=act, state=hidden, taus=taus)

    def _greedy_act(self, logits: torch.Tensor) -> torch.Tensor:
        if self.fused and logits.is_cuda and logits.dim() == 3:
            return iqn_select(logits)[1]
        return self.compute_q_value(logits, None).max(dim=1)[1]

    def _next_rows(self, batch: Batch) -> torch.Tensor:
        """qrdqn.py:60-68 with the two sample sizes: the target network's M quantiles of the
        online network's greedy action at batch.obs_next -- two no-grad forwards and one
        tsrl_iqn_select launch; masked observations take the generic branch."""
        obs_next = batch.obs_next
        masked = isinstance(obs_next, Batch) and "mask" in obs_next
        with torch.no_grad():
            if self.fused and not masked and self._on_device():
                net_in = obs_next.obs if isinstance(obs_next, Batch) and "obs" in obs_next \
                    else obs_next
                info = batch.get("info", Batch())
                (sel, _), _ = self._net_forward("model", net_in, None, info)
                if not hasattr(self, "max_action_num"):
                    self.max_action_num = sel.shape[1]
                ev = self._net_forward("model_old", net_in, None, info)[0][0] if self._target \
                    else None
                return iqn_select(sel, ev, want_act=False, want_row=True)[2]
            if self._target:
                act = self(batch, input="obs_next").act
                next_dist = self(batch, model="model_old", input="obs_next").logits
            else:
                next_batch = self(batch, input="obs_next")
                act, next_dist = next_batch.act, next_batch.logits
            return next_dist[torch.arange(len(act), device=next_dist.device), act, :]

    # -- learn (iqn.py:88-112): DQNPolicy.learn with these hooks ---------------------------------
    def _num_columns(self) -> int:
        """The larger of N and M; without a target network M is the online size."""
        n = self._size_of("model")
        return max(n, self._target_sample_size) if self._target else n

    def _learn_inputs(self, batch: Batch) -> tuple:
        """The fractions of the online forward at obs, drawn ahead of the learn graph."""
        if not self._own_net():
            return ()
        dev = next(self.model.parameters()).device
        return (self._sample_taus((len(batch.returns), self._size_of("model")), dev),)

    def _before_forward(self, info, *extra):
        return extra[0] if extra else None

    def _forward_q(self, obs, info, aux):
        (q, taus), _ = self._net_forward("model", obs, None, info, taus=aux)
        return q, taus

    def _graph_ok(self, obs, n: int) -> bool:
        """A foreign network draws inside its forward: never captured."""
        return self._own_net() and super()._graph_ok(obs, n)

    def _fused_loss(self, q, act, returns, weight, aux, td_out, loss_out):
        return _IQNLoss.apply(q, (act, returns, aux.detach().float().contiguous(), weight,
                                  td_out, loss_out))

    def _learn_torch(self, batch: Batch, weight):
        """The reference's op sequence as written (iqn.py:91-110); returns the loss and the
        priorities that leave as ``batch.weight``."""
        self.optim.zero_grad()
        action_batch = self(batch)
        curr_dist, taus = action_batch.logits, action_batch.taus
        n = len(curr_dist)
        act = torch.as_tensor(batch.act, device=curr_dist.device).reshape(n).long()
        curr_dist = curr_dist[torch.arange(n, device=curr_dist.device), act, :].unsqueeze(2)
        target_dist = torch.as_tensor(batch.returns, device=curr_dist.device).unsqueeze(1)
        dist_diff = F.smooth_l1_loss(target_dist, curr_dist, reduction="none")
        huber_loss = (dist_diff * (taus.unsqueeze(2) - (target_dist - curr_dist).detach().le(0.)
                                   .float()).abs()).sum(-1).mean(1)
        w = 1.0 if weight is None else torch.as_tensor(weight, device=curr_dist.device) \
            .to(curr_dist.dtype)
        loss = (huber_loss * w).mean()
        prio = dist_diff.detach().abs().sum(-1).mean(1)
        loss.backward()
        self.optim.step()
        return loss.detach(), prio
