"""The bindings of csrc/offline.hip that DiscreteBCQPolicy (policy/discrete_bcq.py),
DiscreteCQLPolicy (policy/discrete_cql.py) and DiscreteCRRPolicy (policy/discrete_crr.py) share:
``bcq_select`` and the three fused losses as autograd functions whose forward kernel has already
written the gradients (flat_learn.KernelGradLoss), and the backward + optimiser tail of one
update.  Every loss writes its scalars into one device vector, so learn() reads the host once.
"""
from typing import Optional, Tuple

import torch

from tianshou_amd import _C
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import KernelGradLoss, _partials, _unit_seed, flat_backward

CRR_MODES = {"exp": 0, "binary": 1, "all": 2}


def _table(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a [b, num_actions] table, got {tuple(t.shape)}")
    return t.detach().to(torch.float32).contiguous()


def _same(name: str, b: int, **rows) -> None:
    for k, t in rows.items():
        if t is not None and t.numel() != b:
            raise ValueError(f"{name}: {k} needs {b} elements, got {tuple(t.shape)}")


def bcq_select(q: torch.Tensor, logits: torch.Tensor, log_tau: float,
               q_eval: Optional[torch.Tensor] = None, paper: bool = False
               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(act [b] int64, q_eval[r, act[r]] or None) of discrete_bcq.py:97-99 as one
    tsrl_bcq_select launch.  ``paper`` False: the reference's action (the first allowed one);
    True: the best allowed Q."""
    q, logits = _table(q, "bcq_select q"), _table(logits, "bcq_select logits")
    b, A = q.shape
    if logits.shape != q.shape:
        raise ValueError(f"bcq_select: logits {tuple(logits.shape)} != q {(b, A)}")
    val = None
    if q_eval is not None:
        q_eval = _table(q_eval, "bcq_select q_eval")
        if q_eval.shape != q.shape:
            raise ValueError(f"bcq_select: q_eval {tuple(q_eval.shape)} != q {(b, A)}")
        val = torch.empty(b, dtype=torch.float32, device=q.device)
    act = torch.empty(b, dtype=torch.int64, device=q.device)
    _C.check(_C.lib().tsrl_bcq_select(_C.ptr(q), _C.ptr(logits), float(log_tau), _C.ptr(q_eval),
                                      int(bool(paper)), b, A, _C.ptr(act), _C.ptr(val),
                                      _C.stream_ptr(q.device)), "tsrl_bcq_select")
    return act, val


class BCQLoss(KernelGradLoss):
    """discrete_bcq.py:110-118 as tsrl_bcq_loss_fwd_bwd.  args: (act [b] int64, returns [b]
    f32, weight_reg, loss [4] f32: total, q, i, reg).  Returns the handle to call backward on."""

    @staticmethod
    def forward(ctx, args, q, logits):
        act, returns, weight_reg, loss = args
        x, l = _table(q, "BCQLoss q"), _table(logits, "BCQLoss logits")
        b, A = x.shape
        dev = x.device
        if l.shape != x.shape or loss.numel() != 4:
            raise ValueError("BCQLoss: q and logits need one [b, A] shape, loss four elements")
        _same("BCQLoss", b, act=act, returns=returns)
        grads = [torch.empty_like(x), torch.empty_like(l)]
        _C.check(_C.lib().tsrl_bcq_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(l), _C.ptr(act, torch.int64), _C.ptr(returns, torch.float32),
            float(weight_reg), b, A, _C.ptr(grads[0]), _C.ptr(grads[1]),
            _C.ptr(_partials(b, 3, dev)), _C.ptr(loss, torch.float32), _C.stream_ptr(dev)),
            "tsrl_bcq_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q, logits))
        return torch.empty((), dtype=torch.float32, device=dev)


class CQLLoss(KernelGradLoss):
    """discrete_cql.py:57-76 as tsrl_cql_qr_loss_fwd_bwd.  args: (act [b] int64, returns
    [b, N], tau_hat [N], weight [b] or None, min_q_weight, prio [b], loss [3]: total, qr, cql)."""

    @staticmethod
    def forward(ctx, args, dist):
        act, returns, tau_hat, weight, min_q_weight, prio, loss = args
        x = dist.detach().to(torch.float32).contiguous()
        if x.dim() != 3:
            raise ValueError(f"CQLLoss: need [b, A, N], got {tuple(x.shape)}")
        b, A, N = x.shape
        dev = x.device
        if returns.numel() != b * N or tau_hat.numel() != N or loss.numel() != 3:
            raise ValueError(f"CQLLoss: returns needs {b * N} elements, tau_hat {N}, loss three")
        _same("CQLLoss", b, act=act, weight=weight, prio=prio)
        grad = torch.empty_like(x)
        partials = torch.empty(3 * b, dtype=torch.float64, device=dev)
        _C.check(_C.lib().tsrl_cql_qr_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(act, torch.int64), _C.ptr(returns, torch.float32),
            _C.ptr(tau_hat, torch.float32), _C.ptr(weight, torch.float32), float(min_q_weight),
            b, A, N, _C.ptr(grad), _C.ptr(prio, torch.float32), _C.ptr(partials),
            _C.ptr(loss, torch.float32), _C.stream_ptr(dev)), "tsrl_cql_qr_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, (grad,), (dist,))
        return torch.empty((), dtype=torch.float32, device=dev)


class CRRLoss(KernelGradLoss):
    """discrete_crr.py:88-117 as tsrl_crr_loss_fwd_bwd (a pass for the terms and their batch
    sums, a pass for the gradients: the reference's actor loss is mean(-log_prob) * mean(coef),
    its [b] * [b, 1] product broadcasting to [b, b]).  args: (act [b] int64, target actor
    logits [b, A], target critic q [b, A], rew [b] f32, done [b] uint8, gamma, mode (a key of
    CRR_MODES), beta, ratio_upper_bound, min_q_weight, loss [4]: total, actor, critic, cql)."""

    @staticmethod
    def forward(ctx, args, q, logits):
        act, t_logits, t_q, rew, done, gamma, mode, beta, ub, min_q_weight, loss = args
        x, l = _table(q, "CRRLoss q"), _table(logits, "CRRLoss logits")
        tl, tq = _table(t_logits, "CRRLoss target logits"), _table(t_q, "CRRLoss target q")
        b, A = x.shape
        dev = x.device
        if not l.shape == tl.shape == tq.shape == x.shape or loss.numel() != 4:
            raise ValueError("CRRLoss: the four tables need one [b, A] shape, loss four elements")
        _same("CRRLoss", b, act=act, rew=rew, done=done)
        grads = [torch.empty_like(x), torch.empty_like(l)]
        # two batch means for the gradient pass, then four sums per workgroup
        partials = torch.empty(2 + 4 * int(_C.lib().tsrl_dqn_num_partials(b)),
                               dtype=torch.float64, device=dev)
        _C.check(_C.lib().tsrl_crr_loss_fwd_bwd(
            _C.ptr(x), _C.ptr(l), _C.ptr(act, torch.int64), _C.ptr(tl), _C.ptr(tq),
            _C.ptr(rew, torch.float32), _C.ptr(done, torch.uint8), float(gamma),
            CRR_MODES[mode], float(beta), float(ub), float(min_q_weight), b, A,
            _C.ptr(grads[0]), _C.ptr(grads[1]), _C.ptr(partials),
            _C.ptr(loss, torch.float32), _C.stream_ptr(dev)), "tsrl_crr_loss_fwd_bwd")
        KernelGradLoss.keep(ctx, grads, (q, logits))
        return torch.empty((), dtype=torch.float32, device=dev)


def backward_step(handle: torch.Tensor, fa: Optional[FlatAdam], optim) -> None:
    """The tail of one fused update: backward from a KernelGradLoss handle and one optimiser
    step -- the flat HIP pass with ``fa``, else ``optim.step()``."""
    if fa is None:
        optim.zero_grad()
        handle.backward()
        optim.step()
        return
    with flat_backward((fa,)):
        handle.backward(_unit_seed(handle.device))
    fa.clip_adam(None)  # the reference clips nothing: one optimiser pass
