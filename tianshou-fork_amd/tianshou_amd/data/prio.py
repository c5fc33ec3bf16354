"""PrioritizedReplayBuffer / PrioritizedVectorReplayBuffer (tianshou/data/buffer/prio.py:9-105,
manager.py:195-214, vecbuf.py:40-68) on the device buffers.

The priority sum tree is a device SegmentTree (data/segtree.py); ``init_weight`` on add,
``sample_indices`` (np.random.rand draws, as the reference, times the root, then the
prefix-sum descent), ``get_weight`` and ``update_weight`` run on device tensors.  The running
max / min priority are device scalars, so an update needs no host round trip; the values
follow the reference's dtypes (priorities |w| + eps and their alpha power in the dtype of
the TD errors passed in, importance weights in f64).
"""
from typing import Any, List, Optional, Tuple, Union

import numpy as np
import torch

from tianshou_amd.data.batch import Batch
from tianshou_amd.data.buffer import NstepToken, ReplayBuffer, VectorReplayBuffer
from tianshou_amd.data.segtree import SegmentTree


class _PrioritizedMixin:
    """prio.py:9-105 over the buffer's whole maxsize (manager.py:209-214: the manager owns one
    tree for all sub-buffers)."""

    _prioritized = True

    def _init_prio(self, alpha: float, beta: float, weight_norm: bool) -> None:
        assert alpha > 0.0 and beta >= 0.0
        self._alpha, self._beta = alpha, beta
        self._weight_norm = weight_norm
        self._eps_prio = np.finfo(np.float32).eps.item()
        self._tree = None
        self._max_prio_t = None  # device f64 scalars, created with the tree (value 1.0)
        self._min_prio_t = None
        self.options.update(alpha=alpha, beta=beta)

    @property
    def weight(self) -> SegmentTree:
        if self._tree is None:
            dev = self._ensure_device()
            self._tree = SegmentTree(self.maxsize, dev)
            self._max_prio_t = torch.ones((), dtype=torch.float64, device=dev)
            self._min_prio_t = torch.ones((), dtype=torch.float64, device=dev)
        return self._tree

    @property
    def _max_prio(self) -> float:
        self.weight
        return float(self._max_prio_t.item())

    @property
    def _min_prio(self) -> float:
        self.weight
        return float(self._min_prio_t.item())

    def _idx_dev(self, index) -> torch.Tensor:
        if isinstance(index, torch.Tensor):
            return index.reshape(-1).to(self._ensure_device(), torch.int64)
        return torch.as_tensor(np.asarray(index, np.int64).reshape(-1),
                               device=self._ensure_device())

    def init_weight(self, index) -> None:
        """weight[index] = max_prio ** alpha (prio.py:42-43)."""
        tree = self.weight
        tree.set_dev(self._idx_dev(index), self._max_prio_t ** self._alpha)

    def add(self, batch: Batch, buffer_ids: Optional[Union[np.ndarray, List[int]]] = None
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        ptr, ep_rew, ep_len, ep_idx = super().add(batch, buffer_ids)
        self.init_weight(ptr)
        return ptr, ep_rew, ep_len, ep_idx

    def sample_indices(self, batch_size: int) -> np.ndarray:
        """prio.py:59-64: np.random.rand(batch_size) * total -> prefix-sum descent."""
        if batch_size > 0 and len(self) > 0:
            tree = self.weight
            scalar = torch.as_tensor(np.random.rand(batch_size), device=tree.device) * \
                tree.reduce_dev()
            return tree.prefix_dev(scalar).cpu().numpy()
        return super().sample_indices(batch_size)

    def get_weight_dev(self, index) -> torch.Tensor:
        """(weight[index] / min_prio) ** -beta as a device f64 tensor (prio.py:66-76)."""
        tree = self.weight
        return (tree.get_dev(self._idx_dev(index)) / self._min_prio_t) ** (-self._beta)

    def get_weight(self, index) -> Union[float, np.ndarray]:
        w = self.get_weight_dev(index).cpu().numpy()
        return w if np.ndim(index) else w[0]

    def update_weight(self, index: np.ndarray, new_weight: Union[np.ndarray, torch.Tensor]
                      ) -> None:
        """prio.py:78-89 on device: |w| + eps and its alpha power in w's dtype."""
        tree = self.weight
        w = new_weight if isinstance(new_weight, torch.Tensor) else \
            torch.as_tensor(np.asarray(new_weight))
        w = w.detach().to(tree.device).reshape(-1)
        weight = w.abs() + self._eps_prio
        tree.set_dev(self._idx_dev(index), (weight ** self._alpha).to(torch.float64))
        if weight.numel():
            self._max_prio_t = torch.maximum(self._max_prio_t, weight.max().to(torch.float64))
            self._min_prio_t = torch.minimum(self._min_prio_t, weight.min().to(torch.float64))

    def __getitem__(self, index) -> Batch:
        """prio.py:91-102: the stored keys plus ``weight`` (normalised by its batch maximum
        when weight_norm)."""
        if isinstance(index, slice):
            indices = self.sample_indices(0) if index == slice(None) \
                else self._indices[:len(self)][index]
        else:
            indices = index
        batch = super().__getitem__(indices)
        return self._with_weight(batch, indices.terminal if isinstance(indices, NstepToken)
                                 else indices)

    def _with_weight(self, batch: Batch, indices) -> Batch:
        weight = self.get_weight_dev(indices)
        batch.weight = weight / weight.max() if self._weight_norm and weight.numel() else weight
        return batch

    def sample_nstep(self, batch_size: int, n_step: int, gamma: float
                     ) -> Tuple[Batch, np.ndarray]:
        """The fused sample of the plain buffers plus ``weight``, as ``sample`` returns it."""
        before = self.fused_samples
        batch, indices = super().sample_nstep(batch_size, n_step, gamma)
        if self.fused_samples != before:  # else: sample()'s own __getitem__ added the weight
            batch = self._with_weight(batch, indices)
        return batch, indices

    def set_beta(self, beta: float) -> None:
        self._beta = beta


class PrioritizedReplayBuffer(_PrioritizedMixin, ReplayBuffer):
    """PrioritizedReplayBuffer(size, alpha, beta, weight_norm=True, **kwargs)."""

    def __init__(self, size: int, alpha: float, beta: float, weight_norm: bool = True,
                 **kwargs: Any) -> None:
        ReplayBuffer.__init__(self, size, **kwargs)
        self._init_prio(alpha, beta, weight_norm)


class PrioritizedVectorReplayBuffer(_PrioritizedMixin, VectorReplayBuffer):
    """PrioritizedVectorReplayBuffer(total_size, buffer_num, alpha=, beta=, ...) -- one sum
    tree over the manager's maxsize rows (manager.py:209-214)."""

    def __init__(self, total_size: int, buffer_num: int, alpha: float, beta: float,
                 weight_norm: bool = True, **kwargs: Any) -> None:
        VectorReplayBuffer.__init__(self, total_size, buffer_num, **kwargs)
        self._init_prio(alpha, beta, weight_norm)
