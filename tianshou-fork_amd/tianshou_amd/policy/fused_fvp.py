"""The natural-gradient solve of NPGPolicy / TRPOPolicy on the fused kernels (csrc/fvp.hip).

The reference solves F x = g by 10 conjugate-gradient steps whose products F p are double
backwards through the actor (npg.py:132-181).  For the get_actor_critic actor (diagonal
Gaussian, state-independent log-std) F is the Fisher matrix in closed form, so a solve is

    tsrl_fvp_prepare, tsrl_cg_init, 10 x (tsrl_fvp_apply [2 launches], tsrl_cg_step)

with no autograd graph and no host read: the reference's ``if new_rdotr < residual_tol: break``
is a device flag that turns the remaining launches of the solve into no-ops.
"""
import ctypes

import torch

from tianshou_amd import _C
from tianshou_amd.policy.fused_mlp import FusedActorCritic


class FusedFVP:
    def __init__(self, mlp: FusedActorCritic, actor: torch.nn.Module) -> None:
        self.mlp = mlp
        L = mlp.L
        params = list(actor.parameters())
        sizes = [p.numel() for p in params]

        def off(t: torch.Tensor) -> int:
            i = next(i for i, p in enumerate(params) if p is t)
            return sum(sizes[:i])
        # offsets of the layers in actor.parameters() order (the log-std comes first there)
        self._blocks = [L["sigma"], L["w1a"].weight, L["w1a"].bias, L["w2a"].weight,
                        L["w2a"].bias, L["w3a"].weight, L["w3a"].bias]
        self._offs = [off(t) for t in self._blocks]
        self.P = sum(sizes)
        self._x = None

    def _net(self) -> "_C.FvpNet":
        sg, w1, b1, w2, b2, w3, b3 = (_C.ptr(t.detach()) for t in self._blocks)
        return _C.FvpNet(w1, b1, w2, b2, w3, b3, sg, *self._offs, self.P)

    def _vec(self, key: str) -> torch.Tensor:
        return self.mlp._buf("fvp_" + key, self.P)[:self.P]

    def prepare(self, obs: torch.Tensor) -> None:
        """The actor's activations for the minibatch rows, held until the next prepare."""
        lib = _C.lib()
        x = self.mlp.rows(obs, "xpad_fvp")
        n = x.shape[0]
        nb = int(lib.tsrl_fvp_workspace_bytes(n, self.mlp.D, self.mlp.A))
        ws = self.mlp._buf("fvp_ws", nb, torch.uint8)
        self._x, self._ws, self._nb = x, ws, nb
        self._args = (_C.ptr_rows(x), x.stride(0), n, self.mlp.D, self.mlp.A)
        _C.check(lib.tsrl_fvp_prepare(*self._args, ctypes.byref(self._net()), _C.ptr(ws), nb,
                                      _C.stream_ptr(x.device)), "tsrl_fvp_prepare")

    def apply(self, v: torch.Tensor, damping: float, out: torch.Tensor = None,
              state: torch.Tensor = None) -> torch.Tensor:
        """F v + damping v for the prepared rows (a persistent buffer unless ``out``)."""
        assert self._x is not None, "prepare() first"
        assert v.numel() == self.P and v.dtype == torch.float32
        if out is None:
            out = self._vec("mvp")
        _C.check(_C.lib().tsrl_fvp_apply(
            *self._args, ctypes.byref(self._net()), _C.ptr(v), _C.ptr(out), damping,
            _C.ptr(state), _C.ptr(self._ws), self._nb, _C.stream_ptr(v.device)),
            "tsrl_fvp_apply")
        return out

    def solve(self, b: torch.Tensor, damping: float, nsteps: int = 10,
              residual_tol: float = 1e-10) -> torch.Tensor:
        """npg.py::_conjugate_gradients for the prepared rows; x in a persistent buffer."""
        lib = _C.lib()
        s = _C.stream_ptr(b.device)
        x, r, p, z = (self._vec(k) for k in ("x", "r", "p", "z"))
        state = self.mlp._buf("fvp_state", 2, torch.float64)[:2]
        _C.check(lib.tsrl_cg_init(_C.ptr(b), self.P, _C.ptr(x), _C.ptr(r), _C.ptr(p),
                                  _C.ptr(state), s), "tsrl_cg_init")
        for _ in range(nsteps):
            self.apply(p, damping, z, state)
            _C.check(lib.tsrl_cg_step(_C.ptr(x), _C.ptr(r), _C.ptr(p), _C.ptr(z), self.P,
                                      residual_tol, _C.ptr(state), _C.ptr(self._ws), s),
                     "tsrl_cg_step")
        return x
