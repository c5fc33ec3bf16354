"""What the learn() paths on flat storage (policy/flat_adam.py) share, each defined once: the
target network mirrored into a flat buffer (DQNPolicy._flat_adam, DDPGPolicy._bind), the
bracket around a backward into flat gradient buckets (DQNPolicy._step,
DDPGPolicy._backward_step, FusedLearnMixin._cat_minibatch) and the per-key cache of captured
off-policy updates (DQNPolicy._graph_step, DDPGPolicy._graph_step), and the backward of the
off-policy losses whose kernel has already written the gradients (KernelGradLoss)."""
import contextlib
import warnings
from typing import Callable, Dict, Iterable, Optional, Sequence

import torch

from tianshou_amd import _C
from tianshou_amd.policy.flat_adam import FlatAdam, _slot


def f32_rows(x, dev, n: int) -> torch.Tensor:
    return torch.as_tensor(x, device=dev).reshape(n).to(torch.float32).contiguous()


def mirror_target(old_module: torch.nn.Module, params: Sequence[torch.Tensor],
                  flat_param: torch.Tensor) -> torch.Tensor:
    """Make ``old_module``'s parameters views into a new flat buffer laid out as
    ``flat_param``, the flat storage of the online ``params`` (FlatAdam.flat_param / .params):
    same offsets, shapes and memory formats, the old values kept.  Returns the buffer; a hard
    sync is then one copy, a soft update one launch.  Works on any device."""
    flat_old = torch.empty_like(flat_param)
    o = 0
    for p_old, p in zip(old_module.parameters(), params):
        v = _slot(flat_old, o, p)
        v.copy_(p_old.detach())
        with torch.no_grad():
            p_old.data = v
        o += p.numel()
    return flat_old


def target_mirrored(old_module: torch.nn.Module, flat_old: Optional[torch.Tensor],
                    src: Optional[torch.Tensor], flat_param: Optional[torch.Tensor]) -> bool:
    """``flat_old`` = mirror_target(old_module, ..., src) still mirrors ``flat_param``: that
    is the very buffer ``src``, and every target parameter still lives inside ``flat_old``."""
    if flat_old is None or src is not flat_param:
        return False
    lo = flat_old.data_ptr()
    hi = lo + flat_old.numel() * flat_old.element_size()
    return all(lo <= p.data_ptr() < hi for p in old_module.parameters())


@contextlib.contextmanager
def flat_backward(fas: Iterable[FlatAdam], eager: bool = True):
    """``with flat_backward(fas): loss.backward(...)``.  Eager: autograd hands over each
    gradient and one pass per bucket gathers them into the flat buckets ``fas``; under graph
    capture (or ``eager=False``) it accumulates into the zeroed buckets in place.  The
    optimiser passes stay with the caller."""
    gather = eager and not torch.cuda.is_current_stream_capturing()
    for fa in fas:
        if gather:
            fa.release_grads()
        else:
            fa.zero_grad()
    yield
    if gather:
        for fa in fas:
            fa.gather_grads()


_UNIT = {}


def _unit_seed(dev: torch.device) -> torch.Tensor:
    """A constant f32 1.0 on dev, the seed gradient of the Categorical minibatch's
    loss.backward(): it spares autograd's ones_like fill, and _CatPPOLoss recognises it and
    skips two scaling passes (round 6).  Never written."""
    t = _UNIT.get(dev)
    if t is None:
        t = _UNIT[dev] = torch.ones((), dtype=torch.float32, device=dev)
    return t


def _is_unit_seed(g: torch.Tensor) -> bool:
    t = _UNIT.get(g.device)
    return t is not None and g.dim() == 0 and g.data_ptr() == t.data_ptr()


class KernelGradLoss(torch.autograd.Function):
    """Base of the off-policy losses whose forward kernel writes the gradients as well:
    ``forward(ctx, args, *inputs)`` ends with ``KernelGradLoss.keep(ctx, grads, inputs)`` and
    returns the scalar handle to call backward on."""

    @staticmethod
    def keep(ctx, grads: Sequence[torch.Tensor], inputs: Sequence[torch.Tensor]) -> None:
        ctx.save_for_backward(*grads)
        ctx.meta = [(t.shape, t.dtype) for t in inputs]

    @staticmethod
    def backward(ctx, g):
        grads = ctx.saved_tensors
        if not _is_unit_seed(g):  # backward(UNIT): the kernel's gradients as they are
            grads = [t * g for t in grads]
        return (None, *(t.view(shape).to(dtype) for t, (shape, dtype) in zip(grads, ctx.meta)))


def _partials(b: int, per_row: int, dev) -> Optional[torch.Tensor]:
    """The f64 scratch of a loss kernel with ``per_row`` sums over ``b`` rows (csrc/loss_sum.h):
    None while one workgroup covers the batch."""
    nparts = int(_C.lib().tsrl_ddpg_num_partials(b))
    return torch.empty(per_row * nparts, dtype=torch.float64, device=dev) if nparts > 1 else None


def replay_learn_graph(cache: Dict[tuple, dict], key: tuple, addr: tuple, inputs: Sequence,
                       outputs: Callable, step: Callable, capture: Callable):
    """One update replayed from the HIP graph that ``cache`` holds under ``key``, captured now
    if it holds none.  ``addr``: the addresses every graph of the cache is tied to (the cache
    is emptied first if they moved).  ``inputs``: the live inputs (None entries stay None),
    cloned into the static inputs at capture and copied there before a replay.  ``outputs()``
    allocates the static (td, loss); ``step(static, td, loss)`` runs the update on them inside
    ``capture(graph)``, the policy's own capture context.  Returns (loss, a copy of td) -- or
    None when the capture raised RuntimeError: one warning, the cache emptied, and the caller
    latches the failure and stays eager."""
    if cache and next(iter(cache.values()))["addr"] != addr:
        cache.clear()
    st = cache.get(key)
    if st is None:
        static = [None if a is None else a.clone() for a in inputs]
        td, loss = outputs()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            with capture(graph):
                step(static, td, loss)
        except RuntimeError as err:
            warnings.warn(f"learn-graph capture failed, running updates eagerly: {err}")
            cache.clear()
            torch.cuda.synchronize()
            return None
        st = cache[key] = dict(addr=addr, graph=graph, static=static, td=td, loss=loss)
    else:
        for d, a in zip(st["static"], inputs):
            if d is not None:
                d.copy_(a)
    st["graph"].replay()
    return st["loss"], st["td"].clone()
