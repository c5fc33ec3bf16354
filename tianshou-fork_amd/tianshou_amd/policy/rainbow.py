"""RainbowPolicy (tianshou/policy/modelfree/rainbow.py:8-39): Rainbow DQN, arXiv:1710.02298, as
C51Policy over a network of NoisyLinear layers (utils/net.py ``Net(dueling_param=...)`` with
noisy Q / V heads, utils/net_atari.py ``Rainbow``).

learn() resamples the noise of both networks (``sample_noise``: the reference's ``torch.randn``
calls, then one tsrl_noisy_eps launch per network), puts the target network in training mode so
that its noise takes effect, and runs C51Policy.learn.  The noise is fixed for the whole update,
so the effective parameters mu + sigma * eps of every noisy layer of both networks are built
once, by one tsrl_noisy_weights launch ahead of the update's three forwards, instead of three
torch launches per layer and forward.  That launch is the first node of the learn graph; the
draw stays outside it and the ``eps_*`` buffers, which keep their addresses, are the graph's
static random input.  The dueling combine and the softmax are tsrl_dueling_fwd / _bwd, the sigma
gradients tsrl_noisy_grads (csrc/noisy.hip).

sync_weight copies the noise buffers with the parameters, as the reference's load_state_dict
does: on an update that syncs, both networks use the online network's noise.

``fused = False`` (also handed to every NoisyLinear and dueling head of the networks) keeps the
reference's op sequence, including its per-forward build of the effective weights: the
comparison leg of tools/rainbow_update_bench.py.
"""
from typing import Any, Dict

import torch

from tianshou_amd.data.batch import Batch
from tianshou_amd.policy.c51 import C51Policy
from tianshou_amd.utils.net import (NoisyLinear, noisy_hold, noisy_layers, prepare_noisy,
                                    sample_noise)


class RainbowPolicy(C51Policy):
    """Constructor arguments, defaults and attributes as C51Policy's (rainbow.py:8-33)."""

    @property
    def fused(self) -> bool:
        return self._fused

    @fused.setter
    def fused(self, value: bool) -> None:
        object.__setattr__(self, "_fused", bool(value))
        for net in (getattr(self, "model", None), getattr(self, "model_old", None)):
            for m in net.modules() if net is not None else ():
                if isinstance(m, NoisyLinear):
                    m.fused = bool(value)
                if hasattr(type(m), "fused_dueling"):
                    m.fused_dueling = bool(value)

    def _nets(self) -> tuple:
        return (self.model, self.model_old) if self._target else (self.model,)

    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        """rainbow.py:35-39."""
        sample_noise(self.model)
        if self._target and sample_noise(self.model_old):
            self.model_old.train()  # so that NoisyLinear takes effect
        return super().learn(batch, **kwargs)

    def sync_weight(self) -> None:
        """dqn.py:81-83 for networks whose only buffers are the noise vectors: one copy between
        the flat parameter buffers and one multi-tensor copy of eps_p / eps_q."""
        fa = self._flat
        noisy, noisy_old = noisy_layers(self.model), noisy_layers(self.model_old)
        if fa is not None and fa.adam_bound(self.optim) and self._old_is_flat(fa) and \
                len(noisy) == len(noisy_old) and \
                sum(1 for _ in self.model.buffers()) == 2 * len(noisy):
            self._old_flat.copy_(fa.flat_param)
            if noisy:
                torch._foreach_copy_([t for m in noisy_old for t in (m.eps_p, m.eps_q)],
                                     [t for m in noisy for t in (m.eps_p, m.eps_q)])
            return
        self.model_old.load_state_dict(self.model.state_dict())

    def _step(self, fa, obs, info, act, returns, weight, *extra, td_out=None, loss_out=None):
        """One build of both networks' effective parameters, then C51Policy's update; what it
        built is not trusted afterwards (the optimiser pass changed mu and sigma)."""
        with noisy_hold(*self._nets()):
            return super()._step(fa, obs, info, act, returns, weight, *extra, td_out=td_out,
                                 loss_out=loss_out)

    def _graph_addrs(self) -> tuple:
        """The noisy layers' tensors, effective parameters included: prepare_noisy's key.  It
        also allocates them and uploads the descriptor table, so the capture does neither."""
        return prepare_noisy(*self._nets())
