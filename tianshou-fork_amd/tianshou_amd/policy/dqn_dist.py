"""What C51Policy (policy/c51.py) and QRDQNPolicy (policy/qrdqn.py) share: the bindings of
csrc/dqn_dist.hip and the DQNPolicy hooks that do not depend on the loss.

``dist_select`` is compute_q_value (c51.py:71, qrdqn.py:73), the greedy action and the gather of
that action's atoms (c51.py:74-81, qrdqn.py:59-68) as one tsrl_dist_select launch; ``_C51Loss``
and ``_QRLoss`` are the two learn() bodies (c51.py:82-102, qrdqn.py:82-93) as one fused
forward + backward kernel each, modelled on dqn.py's ``_DQNLoss``.
"""
from typing import Optional, Tuple

import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.onpolicy import _is_unit_seed


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().float().contiguous()


def dist_select(sel: torch.Tensor, eval_: Optional[torch.Tensor] = None,
                w: Optional[torch.Tensor] = None, want_q: bool = False, want_act: bool = True,
                want_row: bool = False) -> Tuple[Optional[torch.Tensor], ...]:
    """(q [b, A], act [b] int64, row [b, N]) of ``sel`` [b, A, N]; an output not asked for is
    None.  q = (sel * w).sum(2), or sel.mean(2) with ``w`` None; act = its first argmax;
    row = (eval_ if given else sel)[r, act[r], :]."""
    if sel.dim() != 3:
        raise ValueError(f"dist_select: need [b, A, N], got {tuple(sel.shape)}")
    sel = _f32c(sel)
    b, A, N = sel.shape
    dev = sel.device
    if eval_ is not None:
        eval_ = _f32c(eval_)
        if eval_.shape != sel.shape:
            raise ValueError(f"dist_select: eval {tuple(eval_.shape)} != sel {(b, A, N)}")
    if w is not None:
        w = _f32c(w).reshape(-1)
        if w.numel() != N:
            raise ValueError(f"dist_select: w has {w.numel()} elements, need {N}")
    q = torch.empty(b, A, dtype=torch.float32, device=dev) if want_q else None
    act = torch.empty(b, dtype=torch.int64, device=dev) if want_act else None
    row = torch.empty(b, N, dtype=torch.float32, device=dev) if want_row else None
    _C.check(_C.lib().tsrl_dist_select(_C.ptr(sel), _C.ptr(eval_), _C.ptr(w), b, A, N, _C.ptr(q),
                                       _C.ptr(act), _C.ptr(row), _C.stream_ptr(dev)),
             "tsrl_dist_select")
    return q, act, row


class _DistLoss(torch.autograd.Function):
    """The shared shape of the two fused losses: dist is the network's [b, A, N] output;
    returns (loss, per-row vector).  ``vec_out`` / ``loss_out`` (optional) receive the outputs
    in place: the static outputs of a captured graph."""

    @staticmethod
    def _launch(x, args, grad, vec, partials, loss, dev):
        raise NotImplementedError

    @classmethod
    def _run(cls, ctx, dist, ctx_args):
        vec_out, loss_out = ctx_args[-2:]
        dev = dist.device
        x = _f32c(dist)
        if x.dim() != 3:
            raise ValueError(f"{cls.__name__}: need [b, A, N], got {tuple(x.shape)}")
        b = x.shape[0]
        grad = torch.empty_like(x)
        vec = torch.empty(b, dtype=torch.float32, device=dev) if vec_out is None else vec_out
        loss = torch.empty((), dtype=torch.float32, device=dev) if loss_out is None \
            else loss_out
        partials = torch.empty(b, dtype=torch.float64, device=dev) if b > 1 else None
        cls._launch(x, ctx_args[:-2], grad, vec, partials, loss, dev)
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


def _rows(t, b: int, n: int, name: str, dtype=torch.float32):
    if t is not None and (t.numel() != b * n or t.dtype != dtype):
        raise ValueError(f"{name}: need {b * n} elements of {dtype}, got {tuple(t.shape)} "
                         f"{t.dtype}")


class _C51Loss(_DistLoss):
    """c51.py:82-102 as tsrl_c51_loss_fwd_bwd.  ctx_args: (act [b], next_dist [b, N], returns
    [b, N], support [N], weight [b] or None, v_min, v_max, delta_z, ce_out, loss_out); returns
    (loss, cross_entropy [b])."""

    @staticmethod
    def forward(ctx, dist, ctx_args):
        return _C51Loss._run(ctx, dist, ctx_args)

    @staticmethod
    def _launch(x, args, grad, vec, partials, loss, dev):
        act, nxt, returns, support, weight, v_min, v_max, delta_z = args
        b, A, N = x.shape
        _rows(act, b, 1, "_C51Loss act", torch.int64)
        _rows(nxt, b, N, "_C51Loss next_dist")
        _rows(returns, b, N, "_C51Loss returns")
        _rows(support, 1, N, "_C51Loss support")
        _rows(weight, b, 1, "_C51Loss weight")
        _rows(vec, b, 1, "_C51Loss ce_out")
        _C.check(_C.lib().tsrl_c51_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(act), _C.ptr(nxt), _C.ptr(returns), _C.ptr(support),
            _C.ptr(weight), b, A, N, float(v_min), float(v_max), float(delta_z), _C.ptr(grad),
            _C.ptr(vec), _C.ptr(partials), _C.ptr(loss), _C.stream_ptr(dev)),
            "tsrl_c51_loss_fwd_bwd")


class _QRLoss(_DistLoss):
    """qrdqn.py:82-93 as tsrl_qr_loss_fwd_bwd.  ctx_args: (act [b], returns [b, N], tau_hat
    [N], weight [b] or None, prio_out, loss_out); returns (loss, prio [b])."""

    @staticmethod
    def forward(ctx, dist, ctx_args):
        return _QRLoss._run(ctx, dist, ctx_args)

    @staticmethod
    def _launch(x, args, grad, vec, partials, loss, dev):
        act, returns, tau_hat, weight = args
        b, A, N = x.shape
        _rows(act, b, 1, "_QRLoss act", torch.int64)
        _rows(returns, b, N, "_QRLoss returns")
        _rows(tau_hat, 1, N, "_QRLoss tau_hat")
        _rows(weight, b, 1, "_QRLoss weight")
        _rows(vec, b, 1, "_QRLoss prio_out")
        _C.check(_C.lib().tsrl_qr_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(act), _C.ptr(returns), _C.ptr(tau_hat), _C.ptr(weight), b, A, N,
            _C.ptr(grad), _C.ptr(vec), _C.ptr(partials), _C.ptr(loss), _C.stream_ptr(dev)),
            "tsrl_qr_loss_fwd_bwd")


class DistDQNMixin:
    """DQNPolicy hooks common to the policies whose network returns [b, A, N]."""

    def _q_weights(self) -> Optional[torch.Tensor]:
        """The [N] weights that reduce the atoms to a Q-value; None: their mean."""
        raise NotImplementedError

    def _num_columns(self) -> int:
        """N: the atoms or quantiles per action."""
        raise NotImplementedError

    def _fused_learn(self) -> bool:
        """More columns than the loss kernels stage (_C.DIST_MAX_N, their argument error):
        learn() takes the torch formulation.  tsrl_dist_select has no such limit."""
        return super()._fused_learn() and self._num_columns() <= _C.DIST_MAX_N

    def _greedy_act(self, logits: torch.Tensor) -> torch.Tensor:
        if self.fused and logits.is_cuda and logits.dim() == 3:
            return dist_select(logits, None, self._q_weights())[1]
        return self.compute_q_value(logits, None).max(dim=1)[1]

    def _next_rows(self, batch: Batch) -> torch.Tensor:
        """c51.py:74-81 / qrdqn.py:60-68: the atoms of the greedy action at batch.obs_next, the
        action from the online network and the atoms from the target network when there is
        one: one or two no-grad forwards and one tsrl_dist_select launch."""
        obs_next = batch.obs_next
        masked = isinstance(obs_next, Batch) and "mask" in obs_next
        with torch.no_grad():
            if self.fused and not masked:
                net_in = obs_next.obs if isinstance(obs_next, Batch) and "obs" in obs_next \
                    else obs_next
                info = batch.get("info", Batch())
                sel, _ = self.model(net_in, state=None, info=info)
                if sel.is_cuda and sel.dim() == 3:
                    if not hasattr(self, "max_action_num"):
                        self.max_action_num = sel.shape[1]
                    ev = self.model_old(net_in, state=None, info=info)[0] if self._target \
                        else None
                    return dist_select(sel, ev, self._q_weights(), want_act=False,
                                       want_row=True)[2]
            if self._target:
                act = self(batch, input="obs_next").act
                next_dist = self(batch, model="model_old", input="obs_next").logits
            else:
                next_batch = self(batch, input="obs_next")
                act, next_dist = next_batch.act, next_batch.logits
            return next_dist[torch.arange(len(act), device=next_dist.device), act, :]

    def _returns_rows(self, batch: Batch, dev, n: int) -> torch.Tensor:
        return torch.as_tensor(batch.returns, device=dev).reshape(n, -1).to(torch.float32) \
            .contiguous()

    def _loss_weight(self, weight, dev, n: int) -> Optional[torch.Tensor]:
        if weight is None:
            return None
        return torch.as_tensor(weight, device=dev).reshape(n).to(torch.float32).contiguous()
