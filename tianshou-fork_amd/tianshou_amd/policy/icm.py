"""ICMPolicy (tianshou/policy/modelbased/icm.py:12-123, arXiv:1705.05363): a wrapper that adds
the forward model's error, scaled by ``reward_scale``, to the reward the inner policy learns
from, and trains the IntrinsicCuriosityModule after the inner policy's learn().

What ``batch.rew`` holds after ``post_process_fn``: the reference's docstring says the original
reward is restored, but ``Batch(orig_rew=batch.rew)`` keeps the very array that ``batch.rew +=``
then updates in place, so ``orig_rew`` is the sum as well and the "restore" assigns the sum back.
The observable result -- ``batch.rew`` and ``batch.policy.orig_rew`` both hold extrinsic +
intrinsic reward after ``update()`` -- is what this class reproduces: the intrinsic reward is
added in place where ``rew`` lives (a device tensor stays on the device, in its dtype).

``fused`` (default: FUSED_DEFAULT, README: the measured rule): when ``match`` accepts the model
-- forward and inverse model exactly ``[Linear, ReLU, Linear]`` with biases, ``feature_dim ==
hidden == W`` in {64, 128}, ``1 <= action_dim <= 32``, f32 head parameters on one GPU -- and
``optim`` is a plain Adam / RMSprop over exactly ``model.parameters()`` and ``feature_net``
returns 2-D f32 device rows of width W:

* ``process_fn`` runs ``feature_net`` twice with autograd on and ONE launch
  (``tsrl_icm_head_fwd``) on the detached features for ``mse_loss`` and ``act_hat``;
* ``learn`` runs ``tsrl_icm_head_step`` (step + fold: the head's forward recomputed -- its
  weights have not changed since ``process_fn`` --, both losses, the eight head gradients
  written straight into their slots of the flat gradient buffer, ``d_phi1``, ``d_phi2`` and the
  three scalars), then ``torch.autograd.backward((phi1, phi2), (d_phi1, d_phi2))`` accumulates the
  feature net's gradients into the same buffer, one flat optimiser pass steps all of them and
  one device-to-host copy reads the scalars.

Everything else -- ``fused=False``, another activation, width or depth, the Atari head
(feature_dim 3136, hidden 512: library-GEMM shapes), an optimiser the flat pass does not bind,
CPU tensors -- runs the reference's op sequence and none of the kernels.  An action outside
``[0, action_dim)`` raises in ``F.one_hot`` there; on the kernels it makes that row's
``mse_loss``, the three losses and the head gradients NaN and touches no memory outside the
arrays.  The feature net stays a torch module.  Data-parallel ICM is not built: the constructor
raises under an active data-parallel group of more than one rank.
"""
import ctypes
from typing import Any, Dict, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from tianshou_amd import _C
from tianshou_amd.data.batch import Batch, to_numpy, to_torch
from tianshou_amd.dist import default_dp
from tianshou_amd.policy.base import BasePolicy
from tianshou_amd.policy.flat_adam import FlatAdam
from tianshou_amd.policy.flat_learn import flat_backward
from tianshou_amd.policy.fused_mlp import _seq

# the default of ICMPolicy's ``fused`` (README: the measured rule)
FUSED_DEFAULT = True
WIDTHS = (64, 128)
MAX_ACTIONS = 32


def match(model) -> Optional[Dict[str, Any]]:
    """The head of an IntrinsicCuriosityModule with the structure the kernels of csrc/icm.hip
    take (the eight parameters in parameters() order, f32 on one device, W, A), or None.
    ICMPolicy adds that the device is a GPU."""
    from tianshou_amd.utils.net import IntrinsicCuriosityModule
    if not isinstance(model, IntrinsicCuriosityModule):
        return None
    W, A = model.feature_dim, model.action_dim
    if W not in WIDTHS or not isinstance(A, int) or not 1 <= A <= MAX_ACTIONS:
        return None
    blocks = []
    for mlp, din, dout in ((model.forward_model, W + A, W), (model.inverse_model, 2 * W, A)):
        mods = _seq(mlp)
        if mods is None or len(mods) != 3:
            return None
        l1, act, l2 = mods
        if not (isinstance(l1, nn.Linear) and type(act) is nn.ReLU and isinstance(l2, nn.Linear)) \
                or l1.bias is None or l2.bias is None or \
                (l1.in_features, l1.out_features, l2.in_features, l2.out_features) != \
                (din, W, W, dout):
            return None
        blocks += [l1.weight, l1.bias, l2.weight, l2.bias]
    head = list(model.forward_model.parameters()) + list(model.inverse_model.parameters())
    dev = blocks[0].device
    if len(head) != 8 or not all(a is b for a, b in zip(head, blocks)) or \
            not all(p.dtype == torch.float32 and p.device == dev for p in blocks):
        return None
    return {"blocks": blocks, "W": W, "A": A}


class FusedHead:
    """The matched head on csrc/icm.hip: descriptors, workspace, the flat optimiser over all of
    ``model.parameters()`` (the feature net's included)."""

    def __init__(self, layers: Dict[str, Any], model: nn.Module) -> None:
        self.blocks, self.W, self.A = layers["blocks"], layers["W"], layers["A"]
        self.flat = FlatAdam(model.parameters())
        self._ws = None

    def takes(self, phi: torch.Tensor) -> bool:
        return isinstance(phi, torch.Tensor) and phi.dtype == torch.float32 and phi.dim() == 2 \
            and phi.shape[1] == self.W and phi.device == self.blocks[0].device

    def _args(self, phi1, phi2, act):
        net = _C.IcmNet(*(_C.ptr(p.detach()) for p in self.blocks))
        return net, (_C.ptr_rows(phi1), phi1.stride(0), _C.ptr_rows(phi2), phi2.stride(0),
                     _C.ptr(act, torch.int64), phi1.shape[0], self.W, self.A, ctypes.byref(net))

    def forward(self, phi1, phi2, act):
        """mse_loss [M], act_hat [M, A] of the detached feature rows."""
        dev, m = phi1.device, phi1.shape[0]
        mse = torch.empty(m, dtype=torch.float32, device=dev)
        act_hat = torch.empty(m, self.A, dtype=torch.float32, device=dev)
        _net, args = self._args(phi1, phi2, act)
        _C.check(_C.lib().tsrl_icm_head_fwd(*args, _C.ptr(mse), _C.ptr(act_hat),
                                            _C.stream_ptr(dev)), "tsrl_icm_head_fwd")
        return mse, act_hat

    def step(self, phi1, phi2, act, lr_scale: float, weight: float, out3: torch.Tensor):
        """The head's gradients into their slots of the flat gradient buffer (bound by the
        caller), the three scalars into out3; returns d_phi1, d_phi2."""
        lib, dev, m = _C.lib(), phi1.device, phi1.shape[0]
        nb = int(lib.tsrl_icm_head_step_workspace_bytes(m, self.W, self.A))
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        grads = _C.IcmNet(*(_C.ptr(p.grad) for p in self.blocks))
        d1, d2 = torch.empty_like(phi1), torch.empty_like(phi2)
        _net, args = self._args(phi1, phi2, act)
        _C.check(lib.tsrl_icm_head_step(
            *args, ctypes.byref(grads), _C.ptr(d1), _C.ptr(d2), float(lr_scale), float(weight),
            _C.ptr(out3), _C.ptr(self._ws), self._ws.numel(), _C.stream_ptr(dev)),
            "tsrl_icm_head_step")
        return d1, d2


class ICMPolicy(BasePolicy):
    def __init__(self, policy: BasePolicy, model, optim: torch.optim.Optimizer, lr_scale: float,
                 reward_scale: float, forward_loss_weight: float, fused: bool = FUSED_DEFAULT,
                 **kwargs: Any) -> None:
        super().__init__(**kwargs)
        dp = default_dp()
        if dp.active and dp.world > 1:
            raise NotImplementedError(
                "data-parallel ICM is not built: the curiosity step would need the ranks' "
                f"gradients combined (world size {dp.world})")
        self.policy = policy
        self.model = model
        self.optim = optim
        self.lr_scale = lr_scale
        self.reward_scale = reward_scale
        self.forward_loss_weight = forward_loss_weight
        self.fused = fused
        layers = match(model)
        self._head = FusedHead(layers, model) \
            if layers is not None and layers["blocks"][0].is_cuda else None
        self._kept = None  # (mse_loss, phi1, phi2, act) of the fused process_fn, for learn()

    def train(self, mode: bool = True) -> "ICMPolicy":
        self.policy.train(mode)
        self.training = mode
        self.model.train(mode)
        return self

    def forward(self, batch: Batch, state: Optional[Union[dict, Batch, np.ndarray]] = None,
                **kwargs: Any) -> Batch:
        return self.policy.forward(batch, state, **kwargs)

    def exploration_noise(self, act, batch: Batch):
        return self.policy.exploration_noise(act, batch)

    def set_eps(self, eps: float) -> None:
        if hasattr(self.policy, "set_eps"):
            self.policy.set_eps(eps)
        else:
            raise NotImplementedError()

    def _curiosity(self, batch: Batch):
        """mse_loss, act_hat of the batch (icm.py:87): on the kernels when they take it."""
        self._kept = None
        head, m = self._head, self.model
        if not self.fused or head is None or not head.flat.bind_adam(self.optim):
            return m(batch.obs, batch.act, batch.obs_next)
        s1 = torch.as_tensor(batch.obs, device=m.device, dtype=torch.float32)
        s2 = torch.as_tensor(batch.obs_next, device=m.device, dtype=torch.float32)
        phi1, phi2 = m.feature_net(s1), m.feature_net(s2)
        act = torch.as_tensor(batch.act, device=m.device, dtype=torch.long)
        if not (head.takes(phi1) and head.takes(phi2) and act.shape == phi1.shape[:1]):
            # the rest of IntrinsicCuriosityModule.forward, on the features already computed
            phi2_hat = m.forward_model(
                torch.cat([phi1, F.one_hot(act, num_classes=m.action_dim)], dim=1))
            mse_loss = 0.5 * F.mse_loss(phi2_hat, phi2, reduction="none").sum(1)
            return mse_loss, m.inverse_model(torch.cat([phi1, phi2], dim=1))
        act = act.contiguous()
        mse_loss, act_hat = head.forward(phi1.detach(), phi2.detach(), act)
        self._kept = (mse_loss, phi1, phi2, act)
        return mse_loss, act_hat

    def process_fn(self, batch: Batch, buffer, indices: np.ndarray) -> Batch:
        mse_loss, act_hat = self._curiosity(batch)
        batch.policy = Batch(orig_rew=batch.rew, act_hat=act_hat, mse_loss=mse_loss)
        if isinstance(batch.rew, torch.Tensor):
            with torch.no_grad():
                batch.rew += (mse_loss * self.reward_scale).to(
                    device=batch.rew.device, dtype=batch.rew.dtype)
        else:
            batch.rew += to_numpy(mse_loss * self.reward_scale)
        return self.policy.process_fn(batch, buffer, indices)

    def post_process_fn(self, batch: Batch, buffer, indices: np.ndarray) -> None:
        self.policy.post_process_fn(batch, buffer, indices)
        batch.rew = batch.policy.orig_rew  # the module docstring: this is the summed reward

    def _learn_fused(self, res: Dict[str, Any]) -> Dict[str, Any]:
        _mse, phi1, phi2, act = self._kept
        self._kept = None
        head = self._head
        out3 = torch.empty(3, dtype=torch.float32, device=phi1.device)
        head.flat.set_lr()
        with flat_backward([head.flat], eager=False):
            d1, d2 = head.step(phi1.detach(), phi2.detach(), act, self.lr_scale,
                               self.forward_loss_weight, out3)
            roots = [(p, d) for p, d in ((phi1, d1), (phi2, d2)) if p.requires_grad]
            if roots:
                torch.autograd.backward(*zip(*roots))
        head.flat.clip_adam(None)
        loss, forward_loss, inverse_loss = out3.tolist()
        res.update({"loss/icm": loss, "loss/icm/forward": forward_loss,
                    "loss/icm/inverse": inverse_loss})
        return res

    def learn(self, batch: Batch, **kwargs: Any) -> Dict[str, float]:
        if self._kept is not None and batch.policy.mse_loss is not self._kept[0]:
            self._kept = None
            raise RuntimeError(
                "ICMPolicy.learn: batch.policy.mse_loss is not the tensor the fused process_fn "
                "produced; learn() must follow process_fn() on the same batch")
        res = self.policy.learn(batch, **kwargs)
        if self._kept is not None:
            return self._learn_fused(res)
        self.optim.zero_grad()
        act_hat = batch.policy.act_hat
        act = to_torch(batch.act, dtype=torch.long, device=act_hat.device)
        inverse_loss = F.cross_entropy(act_hat, act).mean()
        forward_loss = batch.policy.mse_loss.mean()
        loss = ((1 - self.forward_loss_weight) * inverse_loss +
                self.forward_loss_weight * forward_loss) * self.lr_scale
        loss.backward()
        self.optim.step()
        res.update({"loss/icm": loss.item(), "loss/icm/forward": forward_loss.item(),
                    "loss/icm/inverse": inverse_loss.item()})
        return res
