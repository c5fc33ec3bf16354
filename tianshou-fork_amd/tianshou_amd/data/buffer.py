"""Device-resident VectorReplayBuffer / ReplayBuffer.

API of tianshou/data/buffer/{base,manager,vecbuf}.py (0.5.1): ``add``, ``sample``,
``sample_indices``, ``prev``, ``next``, ``unfinished_index``, ``reset``, ``len``,
``__getitem__`` and attribute access to stored keys.  Layout is the reference's env-major
one: env b owns storage rows [b*S, (b+1)*S), S = ceil(total_size / buffer_num)
(vecbuf.py:35).  Storage lives in HBM (torch tensors on the HIP device); the per-env ring
bookkeeping (_index, _lengths, last_index) is host NumPy, vectorised, and never needs device
data; episode statistics (ep_rew/ep_len/ep_idx) live on device and are updated by the
``tsrl_buffer_add`` kernel.
"""
from typing import Any, List, Optional, Tuple, Union

import numpy as np
import torch

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch, gather_rows

_RESERVED = ("obs", "act", "rew", "terminated", "truncated", "done", "obs_next", "info",
             "policy")


def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
        else torch.device("cuda")


class RingIndex:
    """Host-side ring arithmetic of ReplayBufferManager (manager.py:24-192, base.py:140-214)
    for ``num`` sub-buffers of ``size`` rows.  Pure NumPy: the CPU tests exercise it
    directly; it never touches device data."""

    def __init__(self, size: int, num: int) -> None:
        self.size = int(size)
        self.num = int(num)
        self.maxsize = self.size * self.num
        self.offset = np.arange(self.num, dtype=np.int64) * self.size
        self.reset()

    def reset(self) -> None:
        self.index = np.zeros(self.num, np.int64)
        self.lengths = np.zeros(self.num, np.int64)
        self.last_index = self.offset.copy()

    def advance(self, ids: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """One add for envs ``ids`` (unique; None = all): returns (global ptr, next_rel)."""
        if ids is None:
            rel = self.index.copy()
            self.lengths = np.minimum(self.lengths + 1, self.size)
            self.index = (rel + 1) % self.size
            ptr = rel + self.offset
            self.last_index = ptr.copy()
            return ptr, self.index.copy()
        rel = self.index[ids]
        self.lengths[ids] = np.minimum(self.lengths[ids] + 1, self.size)
        self.index[ids] = (rel + 1) % self.size
        ptr = rel + self.offset[ids]
        self.last_index[ids] = ptr
        return ptr, self.index[ids].copy()

    def uniform_rel(self) -> Optional[int]:
        """The common ring position when every sub-buffer is at the same index."""
        i0 = int(self.index[0])
        if np.all(self.index == i0) and np.all(self.lengths == self.lengths[0]):
            return i0
        return None

    def sample0(self) -> np.ndarray:
        """sample_indices(0): each env's rows in ring order, env-major (manager.py:177-192)."""
        L = self.lengths
        if self.num and np.all(L == L[0]):
            n = int(L[0])
            if n == 0:
                return np.zeros(0, np.int64)
            if n == self.size and not self.index.any():
                # every env full with its cursor at 0 (the on-policy layout after
                # reset_buffer + collect(n_step=maxsize)): storage order.  One read-only
                # arange is kept and handed out again (building 8.4M indices costs ~30 ms
                # of host time per update otherwise).
                ident = getattr(self, "_ident", None)
                if ident is None or len(ident) != self.maxsize:
                    ident = np.arange(self.maxsize, dtype=np.int64)
                    ident.flags.writeable = False
                    self._ident = ident
                return ident
            p = np.arange(n, dtype=np.int64)
            rel = (self.index[:, None] + p[None, :]) % n
            return (rel + self.offset[:, None]).reshape(-1)
        parts = [np.concatenate([np.arange(self.index[b], L[b]), np.arange(self.index[b])])
                 + self.offset[b] for b in range(self.num)]
        return np.concatenate(parts).astype(np.int64)

    def chunk_layout(self) -> Tuple[Optional[int], np.ndarray]:
        """(row_len, lengths): row_len is the common per-env chunk length of sample(0) when
        all non-empty envs have the same length (so every row_len-th sample closes an env's
        segment), else None."""
        nz = self.lengths[self.lengths > 0]
        if len(nz) and np.all(nz == nz[0]):
            return int(nz[0]), self.lengths
        return None, self.lengths

    def is_identity(self) -> bool:
        """sample(0) == arange(maxsize): every env full and at ring position 0."""
        return bool(np.all(self.lengths == self.size) and np.all(self.index == 0))


class NstepToken:
    """The terminal rows next^(n_step-1)(indices) of one fused sample
    (``VectorReplayBuffer.sample_nstep``), handed to a policy's ``target_q_fn`` in place of the
    NumPy indices: ``buffer.get(token, "obs_next")`` and ``buffer[token].obs_next`` return the
    rows the sample kernel gathered already, every other key is gathered at the device
    indices, and ``np.asarray(token)`` still yields the indices (the only device-to-host
    copy, made when someone asks for it)."""

    def __init__(self, terminal: torch.Tensor, obs_next: torch.Tensor) -> None:
        self.terminal = terminal
        self.obs_next = obs_next

    def __len__(self) -> int:
        return int(self.terminal.numel())

    def __array__(self, dtype=None, copy=None) -> np.ndarray:
        arr = self.terminal.cpu().numpy()
        return arr if dtype is None else arr.astype(dtype, copy=False)


class _NstepParts:
    """What the last fused sample left for compute_nstep_return (see sample_nstep)."""
    __slots__ = ("indices", "n_step", "gamma", "token", "ret", "coef", "ring_last")


class VectorReplayBuffer:
    """VectorReplayBuffer(total_size, buffer_num) in HBM (vecbuf.py:15-37)."""

    _reserved_keys = _RESERVED
    fused_samples = 0    # sample_nstep calls that took the one-launch tsrl_replay_sample
    _nstep_parts = None  # the parts of the last of them (one-shot, see take_nstep_parts)
    _ring_cache = None   # (host last_index, host lengths, device last_index, device lengths)
    _nstep_ok_meta = None
    # f32 observation rows wider than this many floats get a 128-byte-multiple storage pitch
    # (see _alloc_storage); None-like large value disables the padding
    PAD_MIN = 96

    def __init__(self, total_size: int, buffer_num: int, stack_num: int = 1,
                 ignore_obs_next: bool = False, save_only_last_obs: bool = False,
                 sample_avail: bool = False, device=None, **kwargs: Any) -> None:
        assert buffer_num > 0
        assert stack_num > 0, "stack_num should be greater than 0"
        self.options = dict(stack_num=stack_num, ignore_obs_next=ignore_obs_next,
                            save_only_last_obs=save_only_last_obs, sample_avail=sample_avail)
        self.stack_num = stack_num
        self.buffer_num = int(buffer_num)
        size = int(np.ceil(total_size / buffer_num))
        self._ring = RingIndex(size, buffer_num)
        self.maxsize = self._ring.maxsize
        self._offset = self._ring.offset
        self._extend_offset = np.concatenate([self._offset, [self.maxsize]])
        self._save_obs_next = not ignore_obs_next
        self._save_only_last_obs = save_only_last_obs
        self._sample_avail = sample_avail
        self._indices = np.arange(self.maxsize)
        self.device = torch.device(device) if device is not None else None
        self._meta = Batch()
        self._dev = None  # device-side episode state, allocated with the storage
        self._last_sample0 = None
        self.obs_chain = True  # see reset()

    # -- bookkeeping views ------------------------------------------------------------------
    @property
    def _lengths(self) -> np.ndarray:
        return self._ring.lengths

    @property
    def last_index(self) -> np.ndarray:
        return self._ring.last_index

    @property
    def _index_per_env(self) -> np.ndarray:
        return self._ring.index

    def __len__(self) -> int:
        return int(self._ring.lengths.sum())

    def __repr__(self) -> str:
        return self.__class__.__name__ + repr(self._meta)[5:]

    def __getattr__(self, key: str) -> Any:
        meta = self.__dict__.get("_meta")
        if meta is not None and key in meta.keys():
            return meta[key]
        raise AttributeError(key)

    # -- storage ------------------------------------------------------------------------------
    def _ensure_device(self):
        if self.device is None:
            self.device = _default_device()
        return self.device

    def _alloc_state(self) -> None:
        if self._dev is not None:
            return
        dev = self._ensure_device()
        n = self.buffer_num
        self._dev = dict(
            offset=torch.as_tensor(self._offset, device=dev),
            ep_rew=torch.zeros(n, dtype=torch.float64, device=dev),
            ep_len=torch.zeros(n, dtype=torch.int64, device=dev),
            ep_idx=torch.zeros(n, dtype=torch.int64, device=dev),
            stat_rew=torch.zeros(self.maxsize, dtype=torch.float64, device=dev),
            stat_len=torch.zeros(self.maxsize, dtype=torch.int64, device=dev),
            stat_idx=torch.zeros(self.maxsize, dtype=torch.int64, device=dev),
        )

    def _alloc_storage(self, obs_shape, obs_dtype, act_shape, act_dtype) -> None:
        """First add allocates ``maxsize`` rows per key (batch.py:94-131 lazy alloc)."""
        if not self._meta.is_empty():
            return
        dev = self._ensure_device()
        self._alloc_state()
        m = self.maxsize
        if self._save_only_last_obs:  # manager.py:127-132: one frame per stored row
            obs_shape = tuple(obs_shape)[1:]

        def obs_storage():
            # wide f32 observation rows (e.g. Humanoid's 376 floats = 1504 B) are stored with
            # a 128-byte-multiple pitch (384 floats) and exposed as the [m, D] view: each row
            # starts on a cache line, so the learn kernels' row gathers fetch whole lines (the
            # layer-1 kernel: 241 -> 219 us per 262144-row minibatch); pad columns stay zero
            shape = (m,) + tuple(obs_shape)
            if obs_dtype == torch.float32 and len(obs_shape) == 1 and \
                    obs_shape[0] > self.PAD_MIN and obs_shape[0] % 32:
                d = int(obs_shape[0])
                return torch.zeros((m, (d + 31) // 32 * 32), dtype=obs_dtype,
                                   device=dev)[:, :d]
            return torch.zeros(shape, dtype=obs_dtype, device=dev)

        meta = Batch(
            obs=obs_storage(),
            act=torch.zeros((m,) + tuple(act_shape), dtype=act_dtype, device=dev),
            rew=torch.zeros(m, dtype=torch.float64, device=dev),
            terminated=torch.zeros(m, dtype=torch.bool, device=dev),
            truncated=torch.zeros(m, dtype=torch.bool, device=dev),
            done=torch.zeros(m, dtype=torch.bool, device=dev),
            info=Batch(env_id=torch.zeros(m, dtype=torch.int64, device=dev)),
        )
        if self._save_obs_next:
            meta.obs_next = obs_storage()
        self._meta = meta

    def reset(self, keep_statistics: bool = False) -> None:
        """manager.py:54-58 (+ base.py:140-146 per sub-buffer)."""
        self._ring.reset()
        # obs_chain: every row since the reset came from a Collector step, so within an
        # episode the stored obs of step t+1 is the stored obs_next of step t (process_fn
        # reuses V(s) for V(s') on that basis).  Cleared by add() of arbitrary batches.
        self.obs_chain = True
        if not keep_statistics and self._dev is not None:
            self._dev["ep_rew"].zero_()
            self._dev["ep_len"].zero_()
            self._dev["ep_idx"].zero_()

    def set_batch(self, batch: Batch) -> None:
        """Manually choose the batch the buffer manages (base.py:141-146; manager.py:64-66
        re-points the sub-buffers at slices of it).  Every key is moved into HBM; the ring
        bookkeeping is left as it is, like the reference's.  Rows written this way carry no
        Collector obs / obs_next chain."""
        batch = batch if isinstance(batch, Batch) else Batch(batch)
        assert len(batch) == self.maxsize and set(batch.keys()).issubset(
            self._reserved_keys), "Input batch doesn't meet ReplayBuffer's data form requirement."
        self._alloc_state()
        meta = Batch()
        def nested(b: Batch) -> Batch:
            # every level of a nested Batch (info / policy sub-dicts) moves to the device
            return Batch({kk: nested(vv) if isinstance(vv, Batch) else self._to_dev(vv)
                          for kk, vv in b.items()})

        for k, v in batch.items():
            if isinstance(v, Batch):
                meta.__dict__[k] = nested(v)
                continue
            t = self._to_dev(v)
            if k == "rew":
                t = t.to(torch.float64)
            elif k in ("terminated", "truncated", "done"):
                t = t.bool()
            elif t.dtype == torch.float64 and k in ("obs", "obs_next", "act"):
                t = t.float()
            meta.__dict__[k] = t
        if "done" not in meta.keys() and "terminated" in meta.keys():
            meta.done = meta.terminated | meta.truncated
        if "info" not in meta.keys():
            meta.info = Batch()
        if "env_id" not in meta.info.keys():  # the add kernel records each row's env id
            meta.info.env_id = torch.zeros(self.maxsize, dtype=torch.int64, device=self.device)
        self._meta = meta
        self.obs_chain = False
        self._last_sample0 = None

    @classmethod
    def from_data(cls, obs, act, rew, terminated, truncated, done, obs_next
                  ) -> "VectorReplayBuffer":
        """base.py:109-132 (the hdf5-free part): a one-env buffer of len(obs) rows managing
        the given arrays, _size = len(obs), cursor at 0."""
        size = len(obs)
        assert all(len(d) == size for d in [obs, act, rew, terminated, truncated, done,
                                            obs_next]), \
            "Lengths of all hdf5 datasets need to be equal."
        buf = cls(size) if cls is not VectorReplayBuffer else cls(size, 1)
        if size == 0:
            return buf
        buf.set_batch(Batch(obs=np.asarray(obs), act=np.asarray(act), rew=np.asarray(rew),
                            terminated=np.asarray(terminated), truncated=np.asarray(truncated),
                            done=np.asarray(done), obs_next=np.asarray(obs_next)))
        buf._ring.lengths[0] = size
        return buf

    # -- pickling (base.py:81-87): storage travels as host arrays, back into HBM on load ----
    def __getstate__(self):
        def host(v):
            if isinstance(v, Batch):
                return {"__batch__": {k: host(x) for k, x in v.items()}}
            return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v
        st = {k: v for k, v in self.__dict__.items()
              if k not in ("_meta", "_dev", "_last_sample0", "device", "_nstep_parts",
                           "_ring_cache", "_nstep_ok_meta")}
        st["_meta"] = host(self._meta)
        st["_dev"] = None if self._dev is None else {k: host(v) for k, v in self._dev.items()}
        return st

    def __setstate__(self, state) -> None:
        dev = _default_device()

        def back(v):
            if isinstance(v, dict) and "__batch__" in v:
                return Batch({k: back(x) for k, x in v["__batch__"].items()})
            return torch.as_tensor(v, device=dev) if isinstance(v, np.ndarray) else v
        meta, d = state.pop("_meta"), state.pop("_dev")
        self.__dict__.update(state)
        self.device = dev
        self._last_sample0 = None
        self._meta = back(meta) if isinstance(meta, dict) else Batch()
        self._dev = None if d is None else {k: back(v) for k, v in d.items()}

    def update(self, buffer) -> np.ndarray:
        raise NotImplementedError  # ReplayBufferManager cannot be updated (manager.py:99-101)

    # -- add ------------------------------------------------------------------------------------
    def _to_dev(self, x, dtype=None):
        dev = self._ensure_device()
        if isinstance(x, torch.Tensor):
            t = x.to(dev)
        else:
            t = torch.as_tensor(np.asarray(x), device=dev)
        if dtype is not None:
            t = t.to(dtype)
        return t.contiguous()

    def add(self, batch: Batch, buffer_ids: Optional[Union[np.ndarray, List[int]]] = None
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """ReplayBufferManager.add (manager.py:104-161).  Returns NumPy
        (ptr, ep_rew, ep_len, ep_idx) like the reference (this reads back the episode stats;
        the Collector uses the fused, sync-free ``_add_step`` instead)."""
        for key in ("obs", "act", "rew", "terminated", "truncated"):
            assert key in batch.keys(), f"missing key {key}"
        self.obs_chain = False
        ids = np.arange(self.buffer_num) if buffer_ids is None else \
            np.asarray(buffer_ids, dtype=np.int64)
        k = len(ids)
        obs = self._to_dev(batch.obs)
        act = self._to_dev(batch.act)
        if obs.dtype == torch.float64:
            obs = obs.float()
        if act.dtype == torch.float64:
            act = act.float()
        if obs.dim() == 1:
            obs = obs.reshape(k)
        self._alloc_storage(obs.shape[1:], obs.dtype, act.shape[1:], act.dtype)
        if self._save_only_last_obs:  # manager.py:127-132
            obs = obs[:, -1].contiguous()
        rew = self._to_dev(batch.rew, torch.float64).reshape(k)
        term = self._to_dev(batch.terminated).reshape(k).bool()
        trunc = self._to_dev(batch.truncated).reshape(k).bool()
        obs_next = None
        if self._save_obs_next and "obs_next" in batch.keys() and \
                not (isinstance(batch.obs_next, Batch) and batch.obs_next.is_empty()):
            obs_next = self._to_dev(batch.obs_next).to(self._meta.obs_next.dtype)
            if self._save_only_last_obs:
                obs_next = obs_next[:, -1].contiguous()
        ptr, next_rel = self._ring.advance(ids)
        out_rew = torch.empty(k, dtype=torch.float64, device=self.device)
        out_len = torch.empty(k, dtype=torch.int64, device=self.device)
        out_idx = torch.empty(k, dtype=torch.int64, device=self.device)
        self._launch_add(
            ids=self._to_dev(ids, torch.int64), k=k, ptr=self._to_dev(ptr, torch.int64),
            next_rel=self._to_dev(next_rel, torch.int64), obs=obs.to(self._meta.obs.dtype),
            act=act.to(self._meta.act.dtype), obs_next_raw=obs_next, rew=rew, term=term,
            trunc=trunc, out=(out_rew, out_len, out_idx))
        # extra keys (info.*, policy.*) by plain device scatter
        for key in ("info", "policy"):
            v = batch.get(key)
            if isinstance(v, Batch) and not v.is_empty():
                self._scatter_extra(key, v, ptr)
        return ptr, out_rew.cpu().numpy(), out_len.cpu().numpy(), out_idx.cpu().numpy()

    def _scatter_extra(self, key: str, value: Batch, ptr: np.ndarray) -> None:
        dst = self._meta.get(key)
        if dst is None or not isinstance(dst, Batch):
            dst = Batch()
            self._meta.__dict__[key] = dst
        pt = torch.as_tensor(ptr, device=self.device)
        for k, v in value.items():
            if isinstance(v, Batch):
                continue
            t = self._to_dev(v)
            if k not in dst.keys():
                dst.__dict__[k] = torch.zeros((self.maxsize,) + tuple(t.shape[1:]),
                                              dtype=t.dtype, device=self.device)
            dst.__dict__[k][pt] = t.to(dst.__dict__[k].dtype)

    def _launch_add(self, *, ids, k, ptr=None, next_rel=None, uniform_rel=0, uniform_next=0,
                    rel_dev=None, obs=None, act=None, obs_next=None, obs_next_raw=None,
                    cur_obs=None, norm=None, rew=None, term=None, trunc=None, out=None,
                    stats=True, norm_snapshot=False, reset_src=None, reset_mask=None,
                    reset_norm=None, rel_next=None, launch: bool = True):
        """One tsrl_buffer_add launch (see include/tsrl.h); returns its argument struct
        (launch=False: only build it, e.g. as the pending add of the fused collect step)."""
        m = self._meta
        d = self._dev
        a = _C.AddArgs()
        a.ids = _C.ptr(ids)
        a.ptr = _C.ptr(ptr)
        a.next_rel = _C.ptr(next_rel)
        a.offset = _C.ptr(d["offset"])
        a.k = k
        a.uniform_rel = uniform_rel
        a.uniform_next = uniform_next
        a.rel_dev = _C.ptr(rel_dev)
        a.ring_size = self._ring.size
        a.obs_row_bytes = m.obs.element_size() * int(np.prod(m.obs.shape[1:]))
        if m.obs.dim() == 2 and m.obs.stride(0) != m.obs.shape[1]:
            a.obs_dst_pitch = m.obs.stride(0) * m.obs.element_size()  # padded storage rows
        if obs is not None:
            a.obs_src, a.obs_src_pitch = self._frame_src(obs, a.obs_row_bytes)
            a.obs_dst = _C.ptr_rows(m.obs)
        has_next = self._save_obs_next and "obs_next" in m.keys()
        if obs_next is not None:  # f32 rows, optionally normalised in-kernel
            a.obs_next_src = _C.ptr(obs_next)
            a.obs_next_dst = _C.ptr_rows(m.obs_next) if has_next else None
            a.cur_obs = _C.ptr(cur_obs)
            a.obs_dim = int(np.prod(m.obs.shape[1:]))
            if norm is not None:
                # norm_snapshot: the statistics after merge2's first (step-batch) update
                a.norm_mean = _C.ptr(norm.snap_mean_t if norm_snapshot else norm.mean_t)
                a.norm_var = _C.ptr(norm.snap_var_t if norm_snapshot else norm.var_t)
                a.norm_eps = float(norm.eps)
                a.norm_clip = float(norm.clip_max or 0.0)
            if reset_mask is not None:
                a.reset_src = _C.ptr(reset_src)
                a.reset_mask = _C.ptr(reset_mask)
                if reset_norm is not None:
                    a.reset_mean = _C.ptr(reset_norm.mean_t)
                    a.reset_var = _C.ptr(reset_norm.var_t)
                    a.norm_eps = float(reset_norm.eps)
                    a.norm_clip = float(reset_norm.clip_max or 0.0)
        a.rel_next = _C.ptr(rel_next)
        if obs_next_raw is not None and has_next:
            a.obs_next_src_raw, a.obs_next_src_pitch = self._frame_src(obs_next_raw,
                                                                       a.obs_row_bytes)
            a.obs_next_dst_raw = _C.ptr_rows(m.obs_next)
        if act is not None:
            a.act_src = _C.ptr(act)
            a.act_dst = _C.ptr(m.act)
        a.act_row_bytes = m.act.element_size() * int(np.prod(m.act.shape[1:]))
        a.rew = _C.ptr(rew)
        a.term = _C.ptr(term)
        a.trunc = _C.ptr(trunc)
        a.rew_dst = _C.ptr(m.rew)
        a.term_dst = _C.ptr(m.terminated)
        a.trunc_dst = _C.ptr(m.truncated)
        a.done_dst = _C.ptr(m.done)
        a.env_id_dst = _C.ptr(m.info.env_id)
        a.ep_rew = _C.ptr(d["ep_rew"])
        a.ep_len = _C.ptr(d["ep_len"])
        a.ep_idx = _C.ptr(d["ep_idx"])
        if out is not None:
            a.out_ep_rew, a.out_ep_len, a.out_ep_idx = (_C.ptr(t) for t in out)
        if stats:
            a.stat_rew = _C.ptr(d["stat_rew"])
            a.stat_len = _C.ptr(d["stat_len"])
            a.stat_idx = _C.ptr(d["stat_idx"])
        if launch:
            _C.check(_C.lib().tsrl_buffer_add(a, _C.stream_ptr(self.device)), "tsrl_buffer_add")
        return a

    def _frame_src(self, x: torch.Tensor, row_bytes: int):
        """(source pointer, row pitch) for a source of stored-row payloads: a plain
        [k, ...] tensor (pitch 0 = row_bytes), or with save_only_last_obs a stacked
        [k, stack, ...] tensor whose LAST frame is stored (manager.py:127-132)."""
        full = x.element_size() * (x[0].numel() if x.shape[0] else 0)
        if not self._save_only_last_obs or full == row_bytes or x.shape[0] == 0:
            return _C.ptr(x), 0
        assert x.is_contiguous() and full == row_bytes * x.shape[1], \
            "save_only_last_obs expects [k, stack, *frame] rows"
        return _C.ptr(x) + (x.shape[1] - 1) * row_bytes, full

    # -- sampling -------------------------------------------------------------------------------
    def sample_indices(self, batch_size: int) -> np.ndarray:
        """manager.py:163-192 (host RNG: the same np.random calls as the reference)."""
        if batch_size < 0:
            return np.array([], int)
        if self._sample_avail and self.stack_num > 1:
            all_indices = self._avail_indices()
            if batch_size == 0:
                return all_indices
            return np.random.choice(all_indices, batch_size)
        if batch_size == 0:
            idx = self._ring.sample0()
            self._last_sample0 = idx  # lets process_fn recognise the sample(0) layout
            return idx
        lengths = self._ring.lengths
        buffer_idx = np.random.choice(self.buffer_num, batch_size, p=lengths / lengths.sum())
        sample_num = np.bincount(buffer_idx, minlength=self.buffer_num)
        sample_num[sample_num == 0] = -1
        parts = []
        for b in range(self.buffer_num):
            bsz = sample_num[b]
            if bsz > 0:
                parts.append(np.random.choice(lengths[b], bsz) + self._offset[b])
            else:
                parts.append(np.array([], int))
        return np.concatenate(parts).astype(np.int64)

    def _ring_sample0_env(self, b: int) -> np.ndarray:
        i, L = self._ring.index[b], self._ring.lengths[b]
        return np.concatenate([np.arange(i, L), np.arange(i)])

    def sample(self, batch_size: int) -> Tuple[Batch, np.ndarray]:
        indices = self.sample_indices(batch_size)
        return self[indices], indices

    # -- fused n-step sample ---------------------------------------------------------------------
    def _can_sample_nstep(self) -> bool:
        """Whether tsrl_replay_sample can serve this buffer: one frame per row, plain tensor
        storage on the device, obs and obs_next laid out alike."""
        m = self._meta
        if self._nstep_ok_meta is m:
            return True
        if self.stack_num != 1 or m.is_empty():
            return False
        need = ("obs", "act", "rew", "terminated", "truncated", "done")
        if any(not isinstance(m.get(k), torch.Tensor) or not m[k].is_cuda for k in need):
            return False
        env_id = m.info.get("env_id") if isinstance(m.get("info"), Batch) else None
        if not isinstance(env_id, torch.Tensor) or env_id.dtype != torch.int64:
            return False
        obs = m.obs
        rows_ok = obs.is_contiguous() or (obs.dim() == 2 and obs.stride(1) == 1
                                          and obs.stride(0) >= obs.shape[1])
        if not rows_ok or not m.act.is_contiguous() or m.rew.dtype != torch.float64 or \
                any(m[k].dtype != torch.bool for k in ("terminated", "truncated", "done")):
            return False
        if self._save_obs_next:
            nxt = m.get("obs_next")
            if not isinstance(nxt, torch.Tensor) or nxt.dtype != obs.dtype or \
                    nxt.shape != obs.shape or nxt.stride() != obs.stride():
                return False
        self._nstep_ok_meta = m
        return True

    def sample_nstep(self, batch_size: int, n_step: int, gamma: float
                     ) -> Tuple[Batch, np.ndarray]:
        """``sample(batch_size)`` for an n-step off-policy update: the same (batch, indices),
        gathered by one tsrl_replay_sample launch that also leaves what
        ``BasePolicy.compute_nstep_return(batch, buffer, indices, ..., gamma, n_step)`` needs
        -- the terminal rows, their next observations, the discounted reward sums and the
        bootstrap factors -- on the device for that call (recognised by the identity of
        ``indices``).  Where the kernel cannot serve the buffer (frame stacks, Batch-valued
        observations, batch_size <= 0) this is ``sample``."""
        indices = self.sample_indices(batch_size)
        if batch_size <= 0 or len(indices) == 0 or not self._can_sample_nstep():
            return self[indices], indices
        return self._gather_nstep(indices, int(n_step), float(gamma)), indices

    def _gather_nstep(self, indices: np.ndarray, n_step: int, gamma: float) -> Batch:
        m, dev = self._meta, self.device
        it = self._index_tensor(indices)
        bsz = it.numel()
        obs_st, act_st = m.obs, m.act

        def rows(st):
            return torch.empty((bsz,) + tuple(st.shape[1:]), dtype=st.dtype, device=dev)

        def vec(dtype):
            return torch.empty(bsz, dtype=dtype, device=dev)
        obs, act, obs_next = rows(obs_st), rows(act_st), rows(obs_st)
        term_next = obs_next if n_step == 1 else rows(obs_st)
        rew, ret, coef = vec(torch.float64), vec(torch.float64), vec(torch.float64)
        terminated, truncated, done = vec(torch.bool), vec(torch.bool), vec(torch.bool)
        env_id, terminal = vec(torch.int64), vec(torch.int64)
        done_st, last, lengths = self._ring_dev()
        a = _C.ReplaySampleArgs()
        a.idx, a.bsz = _C.ptr(it), bsz
        a.done, a.last_index, a.lengths = _C.ptr(done_st), _C.ptr(last), _C.ptr(lengths)
        a.size, a.num = self._ring.size, self.buffer_num
        a.n_step, a.gamma = n_step, gamma
        esz = obs_st.element_size()
        a.obs = _C.ptr_rows(obs_st)
        a.obs_next = _C.ptr_rows(m.obs_next) if self._save_obs_next else None
        a.obs_row_bytes = esz * int(np.prod(obs_st.shape[1:]))
        a.obs_pitch = obs_st.stride(0) * esz if obs_st.dim() >= 2 else esz
        a.act = _C.ptr(act_st)
        a.act_row_bytes = act_st.element_size() * int(np.prod(act_st.shape[1:]))
        a.rew, a.terminated, a.truncated = _C.ptr(m.rew), _C.ptr(m.terminated), \
            _C.ptr(m.truncated)
        a.env_id = _C.ptr(m.info.env_id)
        a.obs_out, a.act_out, a.rew_out = _C.ptr(obs), _C.ptr(act), _C.ptr(rew)
        a.terminated_out, a.truncated_out, a.done_out = _C.ptr(terminated), \
            _C.ptr(truncated), _C.ptr(done)
        a.env_id_out, a.obs_next_out = _C.ptr(env_id), _C.ptr(obs_next)
        a.terminal_out, a.term_obs_next_out = _C.ptr(terminal), _C.ptr(term_next)
        a.ret_out, a.coef_out = _C.ptr(ret), _C.ptr(coef)
        _C.check(_C.lib().tsrl_replay_sample(a, _C.stream_ptr(dev)), "tsrl_replay_sample")
        info = Batch({k: env_id if k == "env_id" else gather_rows(v, it)
                      for k, v in m.info.items() if isinstance(v, torch.Tensor)})
        pol = m.get("policy", Batch())
        policy = Batch({k: gather_rows(v, it) for k, v in pol.items()
                        if isinstance(v, torch.Tensor)}) if not pol.is_empty() else Batch()
        p = _NstepParts()
        p.indices, p.n_step, p.gamma = indices, n_step, gamma
        p.token, p.ret, p.coef, p.ring_last = NstepToken(terminal, term_next), ret, coef, last
        self._nstep_parts = p
        self.fused_samples += 1
        return Batch(obs=obs, act=act, rew=rew, terminated=terminated, truncated=truncated,
                     done=done, obs_next=obs_next, info=info, policy=policy)

    def take_nstep_parts(self, indices, n_step: int, gamma: float):
        """The parts of the fused sample that handed out ``indices`` (that very array), if it
        was made with this n_step and gamma and the ring has not moved since; else None.
        One-shot: the parts are dropped either way."""
        p, self._nstep_parts = self._nstep_parts, None
        if p is None or p.indices is not indices or p.n_step != int(n_step) or \
                p.gamma != float(gamma) or p.ring_last is not self._ring_dev()[1]:
            return None
        return p

    def __getitem__(self, index) -> Batch:
        """base.py:360-389.  With stack_num > 1, obs / obs_next / info / policy come back
        stacked [k, stack_num, ...] through the device prev chain (tsrl_stack_gather)."""
        if isinstance(index, NstepToken):
            if self.stack_num > 1 or self._meta.is_empty():
                return self[np.asarray(index)]
            return self._gather_it(index.terminal, obs_next=index.obs_next)
        if isinstance(index, slice):
            indices = self.sample_indices(0) if index == slice(None) \
                else self._indices[:len(self)][index]
        else:
            indices = np.asarray(index)
        m = self._meta
        if m.is_empty():
            return Batch()
        if self.stack_num > 1:
            return self._getitem_stacked(indices)
        if isinstance(index, np.ndarray) and len(indices) == self.maxsize and \
                self._ring.is_identity() and np.array_equal(indices[:1], [0]) and \
                indices[-1] == self.maxsize - 1:
            view = True  # sample(0) of a full on-policy buffer: storage order, no copy
        else:
            view = False
        if view:
            obs = m.obs
            obs_next = m.obs_next if self._save_obs_next else \
                gather_rows(m.obs, self._step_dev(self._index_tensor(indices), -1))
            return Batch(obs=obs, act=m.act, rew=m.rew, terminated=m.terminated,
                         truncated=m.truncated, done=m.done, obs_next=obs_next,
                         info=Batch(env_id=m.info.env_id), policy=m.get("policy", Batch()))
        return self._gather_it(self._index_tensor(indices))

    def _gather_it(self, it: torch.Tensor, obs_next=None) -> Batch:
        """The stored rows at device indices ``it`` (obs_next: rows gathered already)."""
        m = self._meta
        if obs_next is not None:
            pass
        elif self._save_obs_next:
            obs_next = gather_rows(m.obs_next, it)
        else:
            obs_next = gather_rows(m.obs, self._step_dev(it, -1))
        info = Batch({k: gather_rows(v, it) for k, v in m.info.items()
                      if isinstance(v, torch.Tensor)})
        pol = m.get("policy", Batch())
        policy = Batch({k: gather_rows(v, it) for k, v in pol.items()
                        if isinstance(v, torch.Tensor)}) if not pol.is_empty() else Batch()
        return Batch(obs=gather_rows(m.obs, it), act=gather_rows(m.act, it),
                     rew=gather_rows(m.rew, it), terminated=gather_rows(m.terminated, it),
                     truncated=gather_rows(m.truncated, it), done=gather_rows(m.done, it),
                     obs_next=obs_next, info=info, policy=policy)

    def _index_tensor(self, indices) -> torch.Tensor:
        """Device int64 index tensor; NumPy semantics for the range (IndexError past the end,
        negative indices count from the end)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        if len(idx) and (idx.max() >= self.maxsize or idx.min() < -self.maxsize):
            raise IndexError(f"index out of range for buffer of maxsize {self.maxsize}")
        return torch.as_tensor(idx % self.maxsize if len(idx) else idx, device=self.device)

    # -- episode-aware index stepping and frame stacking (device) -----------------------------
    def _ring_dev(self):
        """(done, last_index, lengths) on the device.  The two small uploads are made once
        per buffer write: they are kept until the host ring differs from what was uploaded."""
        ring, c = self._ring, self._ring_cache
        if c is None or not (np.array_equal(c[0], ring.last_index) and
                             np.array_equal(c[1], ring.lengths)):
            dev = self.device
            host_last, host_len = ring.last_index.copy(), ring.lengths.copy()
            c = (host_last, host_len, torch.as_tensor(host_last, device=dev),
                 torch.as_tensor(host_len, device=dev))
            self._ring_cache = c
        return self._meta.done, c[2], c[3]

    def _step_dev(self, it: torch.Tensor, steps: int) -> torch.Tensor:
        """prev^steps (steps > 0) / next^-steps (steps < 0) of device indices
        (manager.py:259-297) via tsrl_ring_step_index."""
        out = torch.empty_like(it)
        if it.numel() == 0:
            return out
        done, last, lengths = self._ring_dev()
        _C.check(_C.lib().tsrl_ring_step_index(
            _C.ptr(it), it.numel(), _C.ptr(done), _C.ptr(last), _C.ptr(lengths),
            self._ring.size, self.buffer_num, int(steps), _C.ptr(out),
            _C.stream_ptr(self.device)), "tsrl_ring_step_index")
        return out

    def _stack_dev(self, val: torch.Tensor, it: torch.Tensor, stack_num: int,
                   want_chain: bool = False):
        """get(index, key, stack_num) for one stored tensor: [k, stack_num, *row]."""
        k = it.numel()
        out = torch.empty((k, stack_num) + tuple(val.shape[1:]), dtype=val.dtype,
                          device=val.device)
        chain = torch.empty((k, stack_num), dtype=torch.int64, device=val.device) \
            if want_chain else None
        if k == 0:
            return out, chain
        done, last, lengths = self._ring_dev()
        row_bytes = val.element_size() * int(np.prod(val.shape[1:]))
        # padded storage (wide f32 rows 128-byte aligned, obs_storage): rows stride(0) apart
        pitch = val.stride(0) * val.element_size() if val.dim() >= 2 else row_bytes
        _C.check(_C.lib().tsrl_stack_gather_pitched(
            _C.ptr_rows(val), pitch, row_bytes, _C.ptr(it), k, stack_num, _C.ptr(done),
            _C.ptr(last),
            _C.ptr(lengths), self._ring.size, self.buffer_num, _C.ptr(out), _C.ptr(chain),
            _C.stream_ptr(self.device)), "tsrl_stack_gather")
        return out, chain

    def _chain_dev(self, it: torch.Tensor, stack_num: int) -> torch.Tensor:
        chain = torch.empty((it.numel(), stack_num), dtype=torch.int64, device=self.device)
        if it.numel():
            done, last, lengths = self._ring_dev()
            _C.check(_C.lib().tsrl_stack_gather(
                None, 0, _C.ptr(it), it.numel(), stack_num, _C.ptr(done), _C.ptr(last),
                _C.ptr(lengths), self._ring.size, self.buffer_num, None, _C.ptr(chain),
                _C.stream_ptr(self.device)), "tsrl_stack_gather")
        return chain

    def get(self, index, key: str, default_value: Any = None,
            stack_num: Optional[int] = None):
        """base.py:317-358: ``self.key[index]`` stacked over ``stack_num`` frames through
        prev (the newest frame last)."""
        if key not in self._meta.keys() and default_value is not None:
            return default_value
        val = self._meta[key]
        if stack_num is None:
            stack_num = self.stack_num
        if isinstance(index, NstepToken):
            if key == "obs_next" and stack_num == 1:
                return index.obs_next
            it = index.terminal
        else:
            it = self._index_tensor(index)
        if stack_num == 1:
            if isinstance(val, Batch):
                return Batch({k: gather_rows(v, it) for k, v in val.items()
                              if isinstance(v, torch.Tensor)})
            return gather_rows(val, it)
        if isinstance(val, Batch):
            if val.is_empty():
                return Batch()
            chain = self._chain_dev(it, stack_num)
            return Batch({k: v[chain] for k, v in val.items() if isinstance(v, torch.Tensor)})
        out, _ = self._stack_dev(val, it, stack_num)
        return out

    def _getitem_stacked(self, indices) -> Batch:
        m = self._meta
        it = self._index_tensor(indices)
        S = self.stack_num
        obs, chain = self._stack_dev(m.obs, it, S, want_chain=True)
        if self._save_obs_next:
            obs_next, _ = self._stack_dev(m.obs_next, it, S)
        else:  # base.py:380-381: get(next(indices), "obs")
            obs_next, _ = self._stack_dev(m.obs, self._step_dev(it, -1), S)
        info = Batch({k: v[chain] for k, v in m.info.items() if isinstance(v, torch.Tensor)})
        pol = m.get("policy", Batch())
        policy = Batch({k: v[chain] for k, v in pol.items() if isinstance(v, torch.Tensor)}) \
            if not pol.is_empty() else Batch()
        return Batch(obs=obs, act=gather_rows(m.act, it), rew=gather_rows(m.rew, it),
                     terminated=gather_rows(m.terminated, it),
                     truncated=gather_rows(m.truncated, it), done=gather_rows(m.done, it),
                     obs_next=obs_next, info=info, policy=policy)

    def _avail_indices(self) -> np.ndarray:
        """manager.py:165-171 + base.py:291-303: per sub-buffer, the sample(0) rows whose
        stack_num-1 predecessors lie in the same episode."""
        idx = self._ring.sample0()
        if len(idx) == 0 or self._meta.is_empty():
            return np.asarray(idx, np.int64)
        it = torch.as_tensor(np.asarray(idx, np.int64), device=self.device)
        p = self._step_dev(it, max(self.stack_num - 2, 0))
        keep = (p != self._step_dev(p, 1)).cpu().numpy()
        return np.asarray(idx, np.int64)[keep]

    # -- episode-aware index stepping (host API; device done flags) ----------------------------
    def _done_at(self, pos: np.ndarray) -> np.ndarray:
        if self._meta.is_empty():
            return np.zeros(len(pos), bool)
        t = torch.as_tensor(np.asarray(pos, np.int64), device=self.device)
        return self._meta.done[t].cpu().numpy()

    def prev(self, index) -> np.ndarray:
        """manager.py:259-277 (_prev_index)."""
        scalar = np.isscalar(index)
        index = np.atleast_1d(np.asarray(index, np.int64)) % self.maxsize
        b = index // self._ring.size
        start = self._offset[b]
        cur = np.maximum(1, self._ring.lengths[b])
        sub = (index - start - 1) % cur
        end = self._done_at(sub + start) | (sub + start == self._ring.last_index[b])
        out = (sub + end) % cur + start
        return out[0] if scalar else out

    def next(self, index) -> np.ndarray:
        """manager.py:280-297 (_next_index)."""
        scalar = np.isscalar(index)
        index = np.atleast_1d(np.asarray(index, np.int64)) % self.maxsize
        b = index // self._ring.size
        start = self._offset[b]
        cur = np.maximum(1, self._ring.lengths[b])
        end = self._done_at(index) | (index == self._ring.last_index[b])
        out = (index - start + 1 - end) % cur + start
        return out[0] if scalar else out

    def _last_positions(self) -> np.ndarray:
        L = self._ring.lengths
        envs = np.flatnonzero(L > 0)
        return (self._ring.index[envs] - 1) % L[envs] + self._offset[envs]

    def unfinished_index(self) -> np.ndarray:
        """manager.py:68-74 (+ base.py:148-151 per sub-buffer)."""
        last = self._last_positions()
        if len(last) == 0:
            return np.array([], np.int64)
        return last[~self._done_at(last)]

    def _unfinished_device(self) -> torch.Tensor:
        """Device int64 tensor of candidate positions (last rows); masked by ~done."""
        last = torch.as_tensor(self._last_positions(), device=self.device)
        return last[~self._meta.done[last]]


class ReplayBuffer(VectorReplayBuffer):
    """Single ReplayBuffer(size) (base.py:11-389): one sub-buffer; batch sampling uses
    np.random.choice(self._size, batch_size) as base.py:285-286 does."""

    def __init__(self, size: int, stack_num: int = 1, ignore_obs_next: bool = False,
                 save_only_last_obs: bool = False, sample_avail: bool = False, device=None,
                 **kwargs: Any) -> None:
        super().__init__(size, 1, stack_num, ignore_obs_next, save_only_last_obs, sample_avail,
                         device)

    def add(self, batch: Batch, buffer_ids=None):
        """base.py:216-274: a single transition (no batch dim) or a stacked one."""
        stacked = buffer_ids is not None
        if not stacked:
            batch = Batch({k: (np.asarray(v)[None] if not isinstance(v, (Batch, torch.Tensor))
                               else (v.unsqueeze(0) if isinstance(v, torch.Tensor) else v))
                           for k, v in batch.items()})
        ptr, r, ln, i = super().add(batch, [0])
        return ptr, r, ln, i

    @property
    def _size(self) -> int:
        return int(self._ring.lengths[0])

    @property
    def _index(self) -> int:
        return int(self._ring.index[0])

    def sample_indices(self, batch_size: int) -> np.ndarray:
        """base.py:276-305."""
        if self._sample_avail and self.stack_num > 1:
            if batch_size < 0:
                return np.array([], int)
            all_indices = self._avail_indices()
            return all_indices if batch_size == 0 else np.random.choice(all_indices, batch_size)
        if batch_size > 0:
            return np.random.choice(self._size, batch_size)
        if batch_size == 0:
            return np.concatenate([np.arange(self._index, self._size), np.arange(self._index)])
        return np.array([], int)
