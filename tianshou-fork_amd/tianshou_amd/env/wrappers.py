"""VectorEnvNormObs on device (tianshou/env/venv_wrappers.py:65-112): the running statistics
(obs_rms) are updated with the RAW obs of every step/reset, then the obs are normalised with
the updated statistics and clipped to +-10.

ContinuousToDiscrete (tianshou/env/gym_wrappers.py:8-34) over a device vector env: a
MultiDiscrete index per action dimension selects a point of that dimension's linspace mesh."""
from typing import List, Union

import numpy as np
import torch

from tianshou_amd.env.spaces import Box, MultiDiscrete
from tianshou_amd.env.synthetic import DeviceVectorEnv
from tianshou_amd.utils.statistics import DeviceRunningMeanStd


class VectorEnvNormObs:
    is_async = False

    def __init__(self, venv, update_obs_rms: bool = True, exact_obs_rms: bool = False) -> None:
        """``exact_obs_rms`` (build option, default off): obs_rms with the reference's f32
        arithmetic bit for bit (DeviceRunningMeanStd(exact=True)) instead of f64 moments."""
        self.venv = venv
        self.update_obs_rms = update_obs_rms
        dim = int(getattr(venv, "obs_numel"))
        self.obs_rms = DeviceRunningMeanStd(dim, venv.device, exact=exact_obs_rms)

    def __len__(self) -> int:
        return len(self.venv)

    def __getattr__(self, key):
        if key == "venv":
            raise AttributeError(key)
        return getattr(self.venv, key)

    def reset(self, id=None, **kwargs):
        obs, info = self.venv.reset(id, **kwargs)
        flat = obs.reshape(len(obs), -1).float()
        if self.obs_rms and self.update_obs_rms:
            self.obs_rms.update(flat)
        return self.obs_rms.norm(flat).reshape(obs.shape), info

    def step(self, action, id=None):
        obs, rew, term, trunc, info = self.venv.step(action, id)
        flat = obs.reshape(len(obs), -1).float()
        if self.obs_rms and self.update_obs_rms:
            self.obs_rms.update(flat)
        return self.obs_rms.norm(flat).reshape(obs.shape), rew, term, trunc, info

    def set_obs_rms(self, obs_rms) -> None:
        if isinstance(obs_rms, DeviceRunningMeanStd):
            self.obs_rms = obs_rms
        else:  # host RunningMeanStd (e.g. loaded from a reference checkpoint)
            self.obs_rms.load(obs_rms.mean, obs_rms.var, obs_rms.count)

    def get_obs_rms(self):
        return self.obs_rms


class ContinuousToDiscrete(DeviceVectorEnv):
    """gym_wrappers.py:8-34 as a vector-env wrapper over a Box-action device env (the
    reference wraps each gym env; here one wrapper serves all envs of ``venv``).
    ``action_space`` is MultiDiscrete(action_per_dim); ``step(act)`` takes int64 indices
    [k, K], gathers the Box action on the device and forwards it.  The per-dimension meshes are
    the reference's ``np.linspace(lo, hi, a)`` on the host, uploaded once as f32 [K, max(a)]
    (rows of fewer points are padded with NaN, and an index is clamped into the table, so a
    wrong index shows in the observations instead of faulting).  A DeviceVectorEnv itself, it
    hands the Collector's device hooks on to ``venv`` with the action mapped."""

    def __init__(self, venv, action_per_dim: Union[int, List[int]]) -> None:
        self.venv = venv
        space = venv.action_space
        assert isinstance(space, Box)
        low, high = space.low, space.high
        if isinstance(action_per_dim, int):
            action_per_dim = [action_per_dim] * space.shape[0]
        assert len(action_per_dim) == space.shape[0]
        self.action_space = MultiDiscrete(action_per_dim)
        self.mesh = [np.linspace(lo, hi, a) for lo, hi, a in zip(low, high, action_per_dim)]
        table = np.full((len(self.mesh), max(action_per_dim)), np.nan, np.float32)
        for i, m in enumerate(self.mesh):
            table[i, :len(m)] = m
        self.mesh_t = torch.as_tensor(table, device=venv.device)
        self._dims = torch.arange(len(self.mesh), device=venv.device)

    def __getattr__(self, key):
        if key == "venv":
            raise AttributeError(key)
        return getattr(self.venv, key)

    def action(self, act):
        """gym_wrappers.py:29-34 on the device: indices [K] or [k, K] -> f32 Box actions."""
        if act is None:
            return None
        act = torch.as_tensor(act, device=self.mesh_t.device).long()
        assert act.dim() <= 2, f"Unknown action format with shape {tuple(act.shape)}."
        return self.mesh_t[self._dims, act.clamp(0, self.mesh_t.shape[1] - 1)]

    def _step_raw(self, ids, k, obs_out, rew_out, term_out, trunc_out, partials=None,
                  action=None) -> None:
        self.venv._step_raw(ids, k, obs_out, rew_out, term_out, trunc_out, partials,
                            self.action(action))

    def _step_reset_raw(self, k, obs_out, reset_out, rew_out, term_out, trunc_out, done_out,
                        partials=None, partials_reset=None, blk_done=None, action=None) -> None:
        self.venv._step_reset_raw(k, obs_out, reset_out, rew_out, term_out, trunc_out, done_out,
                                  partials, partials_reset, blk_done, action=self.action(action))

    def step(self, action, id=None):
        return self.venv.step(self.action(action), id)
