"""Actor/critic networks with the reference's module layout, so ``state_dict()`` keys match
tianshou 0.5.1 checkpoints (utils/net/common.py:56-285, continuous.py:87-235,
discrete.py:12-121, 319-394).  The GEMMs run through PyTorch-ROCm (hipBLASLt) on the GPU;
NoisyLinear's effective parameters, its sigma gradients and the dueling combine are the kernels
of csrc/noisy.hip; ImplicitQuantileNetwork's cosine embedding is tsrl_iqn_embed_fwd / _bwd and
FractionProposalNetwork's forward tsrl_fqf_propose_fwd (csrc/dqn_dist.hip)."""
import contextlib
from typing import Any, Dict, Optional, Sequence, Tuple, Type, Union

import numpy as np
import torch
from torch import nn

from tianshou_amd import _C

SIGMA_MIN = -20
SIGMA_MAX = 2


def sum_rows(x: torch.Tensor) -> torch.Tensor:
    """x.sum(0) for a [rows, cols] f32 HIP tensor through tsrl_sum_rows_f32 (torch's
    reduction of a [262144, 17] gradient took 0.34 ms; this one reads it at HBM rate)."""
    x = x.contiguous()
    rows, cols = x.shape[0], int(x[0].numel()) if x.dim() > 1 else 1
    out = torch.empty(x.shape[1:], dtype=x.dtype, device=x.device)
    L = _C.lib()
    wsb = int(L.tsrl_sum_rows_workspace_bytes(rows, cols))
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=x.device) if wsb else None
    _C.check(L.tsrl_sum_rows_f32(_C.ptr(x), rows, cols, _C.ptr(out), _C.ptr(ws), wsb,
                                 _C.stream_ptr(x.device)), "tsrl_sum_rows_f32")
    return out


def _split_factor(rows: int) -> int:
    """Split-K factor for the weight-gradient GEMM dW = dY^T X over `rows` minibatch rows."""
    for s in (256, 128, 64, 32, 16):
        if rows % s == 0 and rows // s >= 512:
            return s
    return 1


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b.  The backward's weight gradient reduces over the minibatch rows
    (K = 262144 in the benchmark): as a single GEMM that leaves a handful of output tiles for
    256 CUs (hipBLASLt measured 0.75 ms for [64 x 262144] x [262144 x 376] on MI355X), so it
    is split over K in a batched GEMM and the partial products are summed (0.14 ms)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if bias is not None:
            return torch.addmm(bias, x, weight.t())
        return x @ weight.t()

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        need_x, need_w = ctx.needs_input_grad[:2]
        return _linear_grads(x, weight, gy, need_x, need_w,
                             ctx.has_bias and ctx.needs_input_grad[2])


def _linear_grads(x, weight, gy, need_x: bool, need_w: bool, need_b: bool):
    """(gx, gw, gb) of y = x W^T + b from gy; an entry not needed is None.  _LinearFn's
    backward, shared with NoisyLinear's."""
    gx = gw = gb = None
    if torch.is_grad_enabled():
        # backward of a create_graph pass (NPG/TRPO's KL Hessian-vector products): only
        # differentiable torch ops, so the double backward sees the whole graph
        if need_x:
            gx = gy @ weight
        if need_w:
            gw = gy.t() @ x
        if need_b:
            gb = gy.sum(0)
        return gx, gw, gb
    if need_x:
        gx = gy @ weight
    if need_w:
        s = _split_factor(x.shape[0])
        if s > 1 and x.is_cuda:
            part = torch.bmm(gy.reshape(s, -1, gy.shape[1]).transpose(1, 2),
                             x.reshape(s, -1, x.shape[1]))
            gw = sum_rows(part.reshape(s, -1)).view_as(weight)
        else:
            gw = gy.t() @ x
    if need_b:
        gb = sum_rows(gy) if gy.is_cuda else gy.sum(0)
    return gx, gw, gb


class Linear(nn.Linear):
    """nn.Linear (same parameters / state_dict keys) with the split-K weight gradient."""

    def forward(self, x):
        if x.dim() != 2:
            return super().forward(x)
        return _LinearFn.apply(x, self.weight, self.bias)


class EnsembleLinear(nn.Module):
    """The linear layer of an ensemble of networks (common.py:402-432): ``weight`` [E, in, out]
    and ``bias`` [E, 1, out], initialised by the reference's two ``torch.rand`` calls, so a
    seeded construction and a state_dict equal the reference's.  ``x`` is [b, in] (every member
    sees the same rows) or [E, b, in]; the output is [E, b, out], one batched GEMM."""

    def __init__(self, ensemble_size: int, in_feature: int, out_feature: int,
                 bias: bool = True) -> None:
        super().__init__()
        k = np.sqrt(1.0 / in_feature)  # PyTorch's default initialiser
        weight_data = torch.rand((ensemble_size, in_feature, out_feature)) * 2 * k - k
        self.weight = nn.Parameter(weight_data, requires_grad=True)
        self.bias: Optional[nn.Parameter]
        if bias:
            bias_data = torch.rand((ensemble_size, 1, out_feature)) * 2 * k - k
            self.bias = nn.Parameter(bias_data, requires_grad=True)
        else:
            self.bias = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = torch.matmul(x, self.weight)
        if self.bias is not None:
            x = x + self.bias
        return x


# -- NoisyLinear (utils/net/discrete.py:319-394) ---------------------------------------------------
# The effective parameters W_eff = mu_W + sigma_W * outer(eps_q, eps_p) and b_eff of every fused
# training-mode layer on the GPU are built by ONE tsrl_noisy_weights launch per group of
# networks (refresh_noisy) instead of three torch launches per layer and forward.  A layer trusts
# its W_eff only inside a ``noisy_hold`` scope whose entry built it AND while the data pointers
# and ``_version`` counters of its six tensors are the ones seen then.  Outside a scope nothing
# is trusted: a write through ``p.data`` or through a raw pointer (the flat optimiser pass,
# tsrl_noisy_eps, the flat target copy) bumps no counter, so every scope entry from outside
# rebuilds.  Net.forward and net_atari.Rainbow.forward open a scope around their layers (one
# launch per forward); RainbowPolicy opens one around the three forwards of an update (one
# launch per update, the first node of the learn graph).
_hold_depth = 0
_NOISY_TABLES: Dict[tuple, torch.Tensor] = {}  # descriptor tables by addresses and sizes


class _NoisyLinearFn(torch.autograd.Function):
    """y = x W_eff^T + b_eff over the layer's cached effective parameters.  The backward is
    _LinearFn's (gx, the split-K gW, gb); the gradients of mu_W / mu_bias are gW / gb as they
    stand, those of sigma_W / sigma_bias one tsrl_noisy_grads launch."""

    @staticmethod
    def forward(ctx, x, mu_W, sigma_W, mu_bias, sigma_bias, layer):
        w, b = layer._W_eff, layer._b_eff
        ctx.save_for_backward(x, w, layer.eps_p, layer.eps_q)
        return torch.addmm(b, x, w.t())

    @staticmethod
    def backward(ctx, gy):
        x, w, eps_p, eps_q = ctx.saved_tensors
        need = ctx.needs_input_grad
        fused = not torch.is_grad_enabled() and all(need[1:5])
        gx, gw, gb = _linear_grads(x, w, gy, need[0], need[1] or need[2], need[3] or need[4])
        if not fused:  # a create_graph pass, or frozen parameters: differentiable torch ops
            gsw = gw * eps_q.ger(eps_p) if need[2] else None
            gsb = gb * eps_q if need[4] else None
            return gx, gw if need[1] else None, gsw, gb if need[3] else None, gsb, None
        gw, gb = gw.contiguous(), gb.contiguous()
        gsw, gsb = torch.empty_like(gw), torch.empty_like(gb)
        out_f, in_f = gw.shape
        _C.check(_C.lib().tsrl_noisy_grads(
            _C.ptr(gw), _C.ptr(gb), _C.ptr(eps_p), _C.ptr(eps_q), in_f, out_f, _C.ptr(gsw),
            _C.ptr(gsb), _C.stream_ptr(gw.device)), "tsrl_noisy_grads")
        return gx, gw, gsw, gb, gsb, None


class NoisyLinear(nn.Module):
    """Noisy Networks' factorised-noise linear layer, arXiv:1706.10295 (discrete.py:319-379):
    the reference's parameter and buffer names, ``reset()`` / ``sample()`` draw order and
    ``state_dict()``.  In eval mode the forward uses ``mu_W`` / ``mu_bias`` alone.  In training
    mode on the GPU it runs over the cached effective parameters (see above; they are plain
    attributes, never part of ``state_dict()``, and a ``deepcopy`` gets its own); on CPU
    tensors, or with ``fused = False``, it is the reference's formulation on torch."""

    fused = True

    def __init__(self, in_features: int, out_features: int, noisy_std: float = 0.5) -> None:
        super().__init__()
        self.mu_W = nn.Parameter(torch.empty(out_features, in_features))
        self.sigma_W = nn.Parameter(torch.empty(out_features, in_features))
        self.mu_bias = nn.Parameter(torch.empty(out_features))
        self.sigma_bias = nn.Parameter(torch.empty(out_features))
        self.register_buffer("eps_p", torch.empty(in_features))
        self.register_buffer("eps_q", torch.empty(out_features))
        self.in_features = in_features
        self.out_features = out_features
        self.sigma = noisy_std
        self._W_eff: Optional[torch.Tensor] = None
        self._b_eff: Optional[torch.Tensor] = None
        self._fresh_key = None
        self.reset()
        self.sample()

    def reset(self) -> None:
        bound = 1 / np.sqrt(self.in_features)
        self.mu_W.data.uniform_(-bound, bound)
        self.mu_bias.data.uniform_(-bound, bound)
        self.sigma_W.data.fill_(self.sigma / np.sqrt(self.in_features))
        self.sigma_bias.data.fill_(self.sigma / np.sqrt(self.in_features))

    def f(self, x: torch.Tensor) -> torch.Tensor:
        x = torch.randn(x.size(0), device=x.device)
        return x.sign().mul_(x.abs().sqrt_())

    def sample(self) -> None:
        self.eps_p.copy_(self.f(self.eps_p))
        self.eps_q.copy_(self.f(self.eps_q))

    # -- the effective-parameter cache ------------------------------------------------------------
    def _cacheable(self) -> bool:
        return self.training and self.fused and self.mu_W.is_cuda

    def _tensors(self):
        return (self.mu_W, self.sigma_W, self.mu_bias, self.sigma_bias, self.eps_p, self.eps_q)

    def _state_key(self) -> tuple:
        return tuple((t.data_ptr(), t._version) for t in self._tensors()) + \
            (self._W_eff.data_ptr(), self._b_eff.data_ptr())

    def _is_fresh(self) -> bool:
        return self._W_eff is not None and self._fresh_key == self._state_key()

    def _descriptor(self) -> tuple:
        """The layer's tsrl_noisy_layer words; allocates W_eff / b_eff where the parameters
        live."""
        w = self._W_eff
        if w is None or w.device != self.mu_W.device or w.shape != self.mu_W.shape:
            self._W_eff = torch.empty(self.mu_W.shape, dtype=torch.float32,
                                      device=self.mu_W.device)
            self._b_eff = torch.empty(self.mu_bias.shape, dtype=torch.float32,
                                      device=self.mu_W.device)
            self._fresh_key = None
        return tuple(_C.ptr(t.detach(), torch.float32) for t in self._tensors()) + \
            (self._W_eff.data_ptr(), self._b_eff.data_ptr(), self.in_features, self.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training:
            return torch.nn.functional.linear(x, self.mu_W, self.mu_bias)
        if not (self.fused and x.is_cuda and self.mu_W.is_cuda and x.dtype == torch.float32):
            weight = self.mu_W + self.sigma_W * self.eps_q.ger(self.eps_p)
            bias = self.mu_bias + self.sigma_bias * self.eps_q.clone()
            return torch.nn.functional.linear(x, weight, bias)
        if not (_hold_depth and self._is_fresh()):
            refresh_noisy(self)
        if x.dim() == 2:
            return _NoisyLinearFn.apply(x, self.mu_W, self.sigma_W, self.mu_bias,
                                        self.sigma_bias, self)
        y = _NoisyLinearFn.apply(x.reshape(-1, self.in_features), self.mu_W, self.sigma_W,
                                 self.mu_bias, self.sigma_bias, self)
        return y.view(*x.shape[:-1], self.out_features)


def noisy_layers(*models: nn.Module) -> list:
    return [m for model in models for m in model.modules() if isinstance(m, NoisyLinear)]


def _noisy_table(layers) -> Tuple[torch.Tensor, int, tuple]:
    """(device descriptor table, largest in * out, key) of ``layers``, the table cached by its
    key: the device and the addresses and sizes it holds (it is static device memory: a
    captured launch reads it at every replay, so an entry is never dropped)."""
    dev = layers[0].mu_W.device
    key = (dev.index,) + tuple(m._descriptor() for m in layers)
    table = _NOISY_TABLES.get(key)
    if table is None:
        table = _NOISY_TABLES[key] = torch.tensor(key[1:], dtype=torch.int64).to(dev)
    return table, max(m.in_features * m.out_features for m in layers), key


def prepare_noisy(*models: nn.Module) -> tuple:
    """Allocate what refresh_noisy(*models) needs (effective parameters, descriptor table), so
    that a later call can be captured into a graph; returns the table's key."""
    layers = [m for m in noisy_layers(*models) if m._cacheable()]
    return _noisy_table(layers)[2] if layers else ()


def _refresh_layers(layers) -> None:
    table, max_elems, _ = _noisy_table(layers)
    _C.check(_C.lib().tsrl_noisy_weights(_C.ptr(table), len(layers), max_elems,
                                         _C.stream_ptr(table.device)), "tsrl_noisy_weights")
    for m in layers:
        m._fresh_key = m._state_key()


def refresh_noisy(*models: nn.Module) -> bool:
    """Build W_eff / b_eff of every fused training-mode NoisyLinear on the GPU under ``models``
    from the current parameters and noise: one tsrl_noisy_weights launch.  False if there is
    no such layer."""
    layers = [m for m in noisy_layers(*models) if m._cacheable()]
    if layers:
        _refresh_layers(layers)
    return bool(layers)


@contextlib.contextmanager
def noisy_hold(*models: nn.Module):
    """Inside the scope the NoisyLinear layers of ``models`` compute with the effective
    parameters built at its entry (entered from outside any scope: always rebuilt; nested: only
    if a layer's tensors moved or changed version since)."""
    global _hold_depth
    layers = [m for m in noisy_layers(*models) if m._cacheable()]
    if layers and not (_hold_depth and all(m._is_fresh() for m in layers)):
        _refresh_layers(layers)
    _hold_depth += 1
    try:
        yield
    finally:
        _hold_depth -= 1


def _eps_flat(model: nn.Module, layers) -> torch.Tensor:
    """One flat buffer that every eps_p / eps_q of ``layers`` is a view of, in sample order
    (made on first use, and again if a buffer was moved out of it)."""
    flat = model.__dict__.get("_noisy_eps_flat")
    o, ok = 0, flat is not None and flat.device == layers[0].eps_p.device
    for m in layers:
        for t in (m.eps_p, m.eps_q):
            ok = ok and o + t.numel() <= flat.numel() and \
                t.data_ptr() == flat.data_ptr() + 4 * o
            o += t.numel()
    if ok and o == flat.numel():
        return flat
    flat = torch.empty(o, dtype=torch.float32, device=layers[0].eps_p.device)
    o = 0
    for m in layers:
        for t in (m.eps_p, m.eps_q):
            v = flat[o:o + t.numel()]
            v.copy_(t)
            t.data = v
            o += t.numel()
    model.__dict__["_noisy_eps_flat"] = flat
    return flat


def sample_noise(model: nn.Module) -> bool:
    """discrete.py:382-394: resample every NoisyLinear under ``model``; True if there is one.
    On the GPU (all layers fused and on one device) the reference's ``torch.randn`` calls are
    made in its order and sizes into slices of one staging buffer and ONE tsrl_noisy_eps
    launch writes every eps_p / eps_q, which keep their addresses: a seeded run yields the
    reference's values, and a captured update reads the fresh noise."""
    layers = noisy_layers(model)
    if not layers:
        return False
    dev = layers[0].eps_p.device
    if dev.type != "cuda" or not all(m.fused and m.eps_p.device == dev and
                                     m.eps_q.device == dev for m in layers):
        for m in layers:
            m.sample()
        return True
    flat = _eps_flat(model, layers)
    stage = torch.empty_like(flat)
    o = 0
    for m in layers:
        for n in (m.in_features, m.out_features):
            torch.randn(n, device=dev, out=stage[o:o + n])
            o += n
    _C.check(_C.lib().tsrl_noisy_eps(_C.ptr(stage), o, _C.ptr(flat), _C.stream_ptr(dev)),
             "tsrl_noisy_eps")
    return True


# -- the dueling combine (utils/net/common.py:276-284) ---------------------------------------------
class _DuelingRowTooLarge(Exception):
    pass


class _DuelingFn(torch.autograd.Function):
    """out = q - q.mean(1, keepdim) + v (and a softmax over the last dimension) for q
    [b, A, N] and v [b, N] as tsrl_dueling_fwd / tsrl_dueling_bwd."""

    @staticmethod
    def forward(ctx, q, v, softmax):
        qc, vc = q.detach().float().contiguous(), v.detach().float().contiguous()
        b, A, N = qc.shape
        out = torch.empty_like(qc)
        rc = _C.lib().tsrl_dueling_fwd(_C.ptr(qc), _C.ptr(vc), b, A, N, int(softmax), _C.ptr(out),
                                       _C.stream_ptr(qc.device))
        if rc == _C.ERR_DUELING_ROW:
            raise _DuelingRowTooLarge
        _C.check(rc, "tsrl_dueling_fwd")
        ctx.softmax = int(softmax)
        ctx.v_shape = v.shape
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        (out,) = ctx.saved_tensors
        b, A, N = out.shape
        g = g_out.float().contiguous()
        g_q = torch.empty_like(out)
        g_v = torch.empty(b, N, dtype=torch.float32, device=out.device)
        _C.check(_C.lib().tsrl_dueling_bwd(_C.ptr(g), _C.ptr(out), b, A, N, ctx.softmax,
                                           _C.ptr(g_q), _C.ptr(g_v), _C.stream_ptr(out.device)),
                 "tsrl_dueling_bwd")
        return g_q, g_v.view(ctx.v_shape), None


def dueling_combine(q: torch.Tensor, v: torch.Tensor, softmax: bool,
                    fused: bool = True) -> torch.Tensor:
    """q - q.mean(dim=1, keepdim=True) + v for q [b, A, N] and v [b, 1, N], then a softmax over
    N when asked: one launch each way on the GPU; the torch lines on the CPU, with
    ``fused`` False, and when A * N exceeds the kernels' LDS row (TSRL_DUELING_MAX_ROW)."""
    if fused and q.is_cuda and q.dim() == 3 and v.shape == (q.shape[0], 1, q.shape[2]) and \
            q.dtype == torch.float32 and v.dtype == torch.float32 and q.shape[0] > 0:
        try:
            return _DuelingFn.apply(q, v, softmax)
        except _DuelingRowTooLarge:
            pass
    logits = q - q.mean(dim=1, keepdim=True) + v
    return torch.softmax(logits, dim=-1) if softmax else logits


def miniblock(input_size, output_size=0, norm_layer=None, activation=None,
              linear_layer: Type[nn.Linear] = Linear):
    layers = [linear_layer(input_size, output_size)]
    if norm_layer is not None:
        layers += [norm_layer(output_size)]
    if activation is not None:
        layers += [activation()]
    return layers


class MLP(nn.Module):
    """MLP backbone (common.py:56-150): Linear/activation stack in ``self.model``."""

    def __init__(self, input_dim: int, output_dim: int = 0, hidden_sizes: Sequence[int] = (),
                 norm_layer=None, activation=nn.ReLU, device=None,
                 linear_layer: Type[nn.Linear] = Linear, flatten_input: bool = True):
        super().__init__()
        self.device = device
        sizes = [input_dim] + list(hidden_sizes)
        acts = activation if isinstance(activation, (list, tuple)) else \
            [activation] * len(hidden_sizes)
        norms = norm_layer if isinstance(norm_layer, (list, tuple)) else \
            [norm_layer] * len(hidden_sizes)
        model = []
        for i, (din, dout) in enumerate(zip(sizes[:-1], sizes[1:])):
            model += miniblock(din, dout, norms[i], acts[i], linear_layer)
        if output_dim > 0:
            model += [linear_layer(sizes[-1], output_dim)]
        self.output_dim = output_dim or sizes[-1]
        self.model = nn.Sequential(*model)
        self.flatten_input = flatten_input

    def forward(self, obs):
        obs = torch.as_tensor(obs, device=self.device, dtype=torch.float32)
        if self.flatten_input:
            obs = obs.flatten(1)
        return self.model(obs)


class Net(nn.Module):
    """common.py:161-285.  ``dueling_param = (q_kwargs, v_kwargs)`` adds the dueling heads
    ``Q`` and ``V`` (MLPs over the trunk's output, common.py:242-260); their combine, and the
    softmax after it, are one tsrl_dueling_fwd launch on the GPU (``fused_dueling = False``:
    the torch lines).  NoisyLinear layers anywhere inside compute one forward with one build of
    their effective parameters (noisy_hold)."""

    fused_dueling = True

    def __init__(self, state_shape, action_shape=0, hidden_sizes: Sequence[int] = (),
                 norm_layer=None, activation=nn.ReLU, device="cpu", softmax: bool = False,
                 concat: bool = False, num_atoms: int = 1,
                 dueling_param: Optional[Tuple[Dict[str, Any], Dict[str, Any]]] = None,
                 linear_layer=Linear):
        super().__init__()
        self.device = device
        self.softmax = softmax
        self.num_atoms = num_atoms
        input_dim = int(np.prod(state_shape))
        action_dim = int(np.prod(action_shape)) * num_atoms
        if concat:
            input_dim += action_dim
        self.use_dueling = dueling_param is not None
        output_dim = action_dim if not self.use_dueling and not concat else 0
        self.model = MLP(input_dim, output_dim, hidden_sizes, norm_layer, activation, device,
                         linear_layer)
        self.output_dim = self.model.output_dim
        if self.use_dueling:
            q_kwargs, v_kwargs = dueling_param
            q_output_dim, v_output_dim = 0, 0
            if not concat:
                q_output_dim, v_output_dim = action_dim, num_atoms
            q_kwargs = {**q_kwargs, "input_dim": self.output_dim, "output_dim": q_output_dim,
                        "device": self.device}
            v_kwargs = {**v_kwargs, "input_dim": self.output_dim, "output_dim": v_output_dim,
                        "device": self.device}
            self.Q, self.V = MLP(**q_kwargs), MLP(**v_kwargs)
            self.output_dim = self.Q.output_dim
        else:
            self.Q, self.V = None, None
        self._noisy = bool(noisy_layers(self))

    def forward(self, obs, state: Any = None, **kwargs):
        if self._noisy and self.training:
            with noisy_hold(self):
                return self._forward(obs), state
        return self._forward(obs), state

    def _forward(self, obs):
        logits = self.model(obs)
        batch_size = logits.shape[0]
        if self.use_dueling:
            q, v = self.Q(logits), self.V(logits)
            if self.num_atoms > 1:
                q = q.view(batch_size, -1, self.num_atoms)
                v = v.view(batch_size, -1, self.num_atoms)
                return dueling_combine(q, v, self.softmax, self.fused_dueling)
            logits = dueling_combine(q.unsqueeze(2), v.unsqueeze(2), False,
                                     self.fused_dueling).squeeze(2)
        elif self.num_atoms > 1:
            logits = logits.view(batch_size, -1, self.num_atoms)
        if self.softmax:
            logits = torch.softmax(logits, dim=-1)
        return logits


class _BDQCombineFn(torch.autograd.Function):
    """out = v + s - s.mean(2, keepdim) for s [b, K, A] and v [b] as tsrl_bdq_combine_fwd /
    tsrl_bdq_combine_bwd; with ``want_act`` the second output is the per-branch greedy action
    [b, K] of the rounded out values (None otherwise)."""

    @staticmethod
    def forward(ctx, s, v, want_act):
        sc, vc = s.detach().float().contiguous(), v.detach().float().contiguous()
        b, K, A = sc.shape
        out = torch.empty_like(sc)
        act = torch.empty(b, K, dtype=torch.int64, device=sc.device) if want_act else None
        _C.check(_C.lib().tsrl_bdq_combine_fwd(_C.ptr(sc), _C.ptr(vc), b, K, A, _C.ptr(out),
                                               _C.ptr(act), _C.stream_ptr(sc.device)),
                 "tsrl_bdq_combine_fwd")
        ctx.v_shape = v.shape
        if act is not None:
            ctx.mark_non_differentiable(act)
        return out, act

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, _g_act):
        g = g_out.float().contiguous()
        b, K, A = g.shape
        g_s = torch.empty_like(g)
        g_v = torch.empty(b, dtype=torch.float32, device=g.device)
        _C.check(_C.lib().tsrl_bdq_combine_bwd(_C.ptr(g), b, K, A, _C.ptr(g_s), _C.ptr(g_v),
                                               _C.stream_ptr(g.device)), "tsrl_bdq_combine_bwd")
        return g_s, g_v.view(ctx.v_shape), None


class BranchingNet(nn.Module):
    """Branching dueling Q-network (common.py:435-544, arXiv:1711.08946): a shared trunk
    ``common``, a state-value head ``value`` and one advantage head per action dimension in
    ``branches``, built in the reference's order (a seeded construction is bit-equal and a
    reference ``state_dict`` loads with ``strict=True``).  ``forward`` returns logits
    [b, K, A] = value + advantage - mean of the advantages inside the branch.

    ``norm_args`` / ``act_args`` sit at the reference's positions, but this package's MLP
    takes neither: anything but ``None`` raises ``NotImplementedError`` naming the argument.

    On the GPU the aggregation is one tsrl_bdq_combine_fwd launch (one tsrl_bdq_combine_bwd
    in the backward); without gradients the same launch also writes the greedy action of
    every branch, which BranchingDQNPolicy.forward picks up (``greedy_act``).  The torch lines
    (common.py:537-543) run on the CPU, with ``fused_combine = False`` and for non-f32
    outputs."""

    fused_combine = True

    def __init__(self, state_shape, num_branches: int = 0, action_per_branch: int = 2,
                 common_hidden_sizes=None, value_hidden_sizes=None, action_hidden_sizes=None,
                 norm_layer=None, norm_args=None, activation=nn.ReLU, act_args=None,
                 device="cpu") -> None:
        super().__init__()
        if norm_args is not None:
            raise NotImplementedError("BranchingNet: norm_args is not supported (MLP builds "
                                      "norm_layer(output_size))")
        if act_args is not None:
            raise NotImplementedError("BranchingNet: act_args is not supported (MLP builds "
                                      "activation())")
        common_hidden_sizes = common_hidden_sizes or []
        value_hidden_sizes = value_hidden_sizes or []
        action_hidden_sizes = action_hidden_sizes or []
        self.device = device
        self.num_branches = num_branches
        self.action_per_branch = action_per_branch
        self.common = MLP(int(np.prod(state_shape)), 0, common_hidden_sizes, norm_layer,
                          activation, device)
        self.value = MLP(common_hidden_sizes[-1], 1, value_hidden_sizes, norm_layer, activation,
                         device)
        self.branches = nn.ModuleList([
            MLP(common_hidden_sizes[-1], action_per_branch, action_hidden_sizes, norm_layer,
                activation, device) for _ in range(self.num_branches)])
        self._greedy = None  # (logits, act) of the last no-grad fused forward

    def greedy_act(self, logits: torch.Tensor) -> Optional[torch.Tensor]:
        """The [b, K] greedy actions the combine launch wrote beside ``logits`` (None when
        ``logits`` is not the last no-grad fused forward's output)."""
        g = self._greedy
        return g[1] if g is not None and g[0] is logits else None

    def forward(self, obs, state: Any = None, **kwargs):
        common_out = self.common(obs)
        value_out = self.value(common_out)
        action_scores = torch.stack([b(common_out) for b in self.branches], 1)
        self._greedy = None
        if self.fused_combine and action_scores.is_cuda and action_scores.shape[0] > 0 and \
                action_scores.dtype == torch.float32 and value_out.dtype == torch.float32:
            want_act = not (torch.is_grad_enabled() and
                            (action_scores.requires_grad or value_out.requires_grad))
            logits, act = _BDQCombineFn.apply(action_scores, value_out.reshape(-1), want_act)
            if want_act:
                self._greedy = (logits, act)
            return logits, state
        value_out = torch.unsqueeze(value_out, 1)
        action_scores = action_scores - torch.mean(action_scores, 2, keepdim=True)
        return value_out + action_scores, state


def _module_device(m: nn.Module):
    try:
        return next(m.parameters()).device
    except StopIteration:
        return None


class _PreprocessWrapper(nn.Module):
    """continuous.py:13-30: the preprocess net is registered under two names."""

    def __init__(self, preprocess_net: nn.Module, device=None):
        super().__init__()
        device = device if device else _module_device(preprocess_net)
        preprocess_net.to(device)
        self.device = device
        self.preprocess_net = preprocess_net
        self.preprocess = preprocess_net


class ActorProb(_PreprocessWrapper):
    """Gaussian actor (continuous.py:153-235).  With ``conditioned_sigma=False`` the log-std
    ``sigma_param`` is state-independent, which is what the fused HIP PPO loss consumes."""

    def __init__(self, preprocess_net, action_shape, hidden_sizes=(), max_action=1.0,
                 device="cpu", unbounded=False, conditioned_sigma=False,
                 preprocess_net_output_dim=None):
        super().__init__(preprocess_net, device=device)
        if unbounded:
            max_action = 1.0
        self.output_dim = int(np.prod(action_shape))
        input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.mu = MLP(input_dim, self.output_dim, hidden_sizes, device=self.device)
        self._c_sigma = conditioned_sigma
        if conditioned_sigma:
            self.sigma = MLP(input_dim, self.output_dim, hidden_sizes, device=self.device)
        else:
            self.sigma_param = nn.Parameter(torch.zeros(self.output_dim, 1))
        self.max_action = max_action
        self._unbounded = unbounded

    def forward_mu(self, obs):
        logits, _ = self.preprocess(obs, None)
        mu = self.mu(logits)
        if not self._unbounded:
            mu = self.max_action * torch.tanh(mu)
        return mu

    def forward(self, obs, state=None, info: Dict[str, Any] = {}):
        logits, hidden = self.preprocess(obs, state)
        mu = self.mu(logits)
        if not self._unbounded:
            mu = self.max_action * torch.tanh(mu)
        if self._c_sigma:
            sigma = torch.clamp(self.sigma(logits), min=SIGMA_MIN, max=SIGMA_MAX).exp()
        else:
            shape = [1] * len(mu.shape)
            shape[1] = -1
            sigma = (self.sigma_param.view(shape) + torch.zeros_like(mu)).exp()
        return (mu, sigma), state


class Actor(_PreprocessWrapper):
    """Deterministic actor (continuous.py:31-84): preprocess -> MLP ``last`` ->
    max_action * tanh.  DDPGPolicy's and TD3Policy's actor."""

    def __init__(self, preprocess_net, action_shape, hidden_sizes=(), max_action=1.0,
                 device="cpu", preprocess_net_output_dim=None):
        super().__init__(preprocess_net, device=device)
        self.output_dim = int(np.prod(action_shape))
        input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.last = MLP(input_dim, self.output_dim, hidden_sizes, device=self.device)
        self.max_action = max_action

    def forward(self, obs, state=None, info: Dict[str, Any] = {}):
        logits, hidden = self.preprocess(obs, state)
        logits = self.max_action * torch.tanh(self.last(logits))
        return logits, hidden


class Critic(_PreprocessWrapper):
    """V(s) head (continuous.py:87-150)."""

    def __init__(self, preprocess_net, hidden_sizes=(), device=None,
                 preprocess_net_output_dim=None, linear_layer=Linear, flatten_input=True):
        super().__init__(preprocess_net, device=device)
        self.output_dim = 1
        input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.last = MLP(input_dim, 1, hidden_sizes, device=self.device,
                        linear_layer=linear_layer, flatten_input=flatten_input)

    def forward(self, obs, act=None, info: Dict[str, Any] = {}):
        obs = torch.as_tensor(obs, device=self.device, dtype=torch.float32).flatten(1)
        if act is not None:
            act = torch.as_tensor(act, device=self.device, dtype=torch.float32).flatten(1)
            obs = torch.cat([obs, act], dim=1)
        logits, _ = self.preprocess(obs)
        return self.last(logits)


class DiscreteActor(nn.Module):
    """Softmax actor (utils/net/discrete.py:12-71): preprocess -> MLP -> softmax unless
    softmax_output=False.  Module layout (``preprocess``, ``last``) as the reference's, so
    state_dicts interchange."""

    def __init__(self, preprocess_net, action_shape, hidden_sizes=(), softmax_output=True,
                 preprocess_net_output_dim=None, device="cpu"):
        super().__init__()
        self.device = device
        self.preprocess = preprocess_net
        self.output_dim = int(np.prod(action_shape))
        input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.last = MLP(input_dim, self.output_dim, hidden_sizes, device=self.device)
        self.softmax_output = softmax_output

    def forward(self, obs, state=None, info: Dict[str, Any] = {}):
        logits, hidden = self.preprocess(obs, state)
        logits = self.last(logits)
        if self.softmax_output:
            logits = torch.softmax(logits, dim=-1)
        return logits, hidden


class DiscreteCritic(nn.Module):
    """V(s) head of discrete-action policies (utils/net/discrete.py:74-121): the observation
    goes to the preprocess net unchanged (a conv trunk sees its frame stack)."""

    def __init__(self, preprocess_net, hidden_sizes=(), last_size: int = 1,
                 preprocess_net_output_dim=None, device="cpu"):
        super().__init__()
        self.device = device
        self.preprocess = preprocess_net
        self.output_dim = last_size
        input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.last = MLP(input_dim, last_size, hidden_sizes, device=self.device)

    def forward(self, obs, **kwargs: Any):
        logits, _ = self.preprocess(obs, state=kwargs.get("state", None))
        return self.last(logits)


class _IQNEmbedFn(torch.autograd.Function):
    """out [b * N, D] = h[r] * relu(cosines(taus) W^T + bias): the cosine embedding and its
    Hadamard product with the state embedding as tsrl_iqn_embed_fwd / tsrl_iqn_embed_bwd.  The
    weight gradient is _linear_grads' (g_z, cosine features); the bias gradient comes out of the
    backward kernel's own f64 fold (at one-feature shapes an f32 row sum of g_z deviated from
    f64 by 20 x what torch's own sum did); taus get none."""

    @staticmethod
    def forward(ctx, h, taus, weight, bias):
        hc, tc = h.detach().float().contiguous(), taus.detach().float().contiguous()
        wc, bc = weight.detach().contiguous(), bias.detach().contiguous()
        (b, D), N, C = hc.shape, tc.shape[1], wc.shape[1]
        if tc.dim() != 2 or tc.shape[0] != b or wc.shape != (D, C) or bc.shape != (D,):
            raise ValueError(f"_IQNEmbedFn: h {tuple(hc.shape)}, taus {tuple(tc.shape)}, weight "
                             f"{tuple(wc.shape)}, bias {tuple(bc.shape)} do not fit")
        e = torch.empty(b * N, D, dtype=torch.float32, device=hc.device)
        out = torch.empty_like(e)
        _C.check(_C.lib().tsrl_iqn_embed_fwd(
            _C.ptr(hc), _C.ptr(tc), _C.ptr(wc, torch.float32), _C.ptr(bc, torch.float32), b, N,
            D, C, _C.ptr(e), _C.ptr(out), _C.stream_ptr(hc.device)), "tsrl_iqn_embed_fwd")
        ctx.save_for_backward(h, tc, e, weight, bias)
        return out

    @staticmethod
    def backward(ctx, g_out):
        h, taus, e, weight, bias = ctx.saved_tensors
        need_h, _, need_w, need_b = ctx.needs_input_grad
        (b, D), N, C = h.shape, taus.shape[1], weight.shape[1]
        if torch.is_grad_enabled():
            # a create_graph pass: the reference's op sequence from the inputs again, so the
            # double backward sees the whole graph
            emb = torch.relu(torch.addmm(bias, CosineEmbeddingNetwork.cosines(taus, C),
                                         weight.t())).view(b, N, D)
            out = (h.unsqueeze(1) * emb).view(b * N, D)
            ins = [t for t, need in ((h, need_h), (weight, need_w), (bias, need_b)) if need]
            grads = iter(torch.autograd.grad(out, ins, g_out, create_graph=True))
            return (next(grads) if need_h else None, None, next(grads) if need_w else None,
                    next(grads) if need_b else None)
        h_dtype, h = h.dtype, h.detach().float().contiguous()
        g = g_out.float().contiguous()
        g_h = torch.empty_like(h)
        g_z = torch.empty_like(e)
        cos = torch.empty(b * N, C, dtype=torch.float32, device=h.device) if need_w else None
        gb = torch.empty(D, dtype=torch.float32, device=h.device) if need_b else None
        part = torch.empty(b, D, dtype=torch.float64, device=h.device) if need_b else None
        _C.check(_C.lib().tsrl_iqn_embed_bwd(
            _C.ptr(g), _C.ptr(e), _C.ptr(h), _C.ptr(taus), b, N, D, C, _C.ptr(g_h), _C.ptr(g_z),
            _C.ptr(cos), _C.ptr(part), _C.ptr(gb), _C.stream_ptr(h.device)),
            "tsrl_iqn_embed_bwd")
        _, gw, _ = _linear_grads(cos, weight, g_z, False, need_w, False)
        return g_h.to(h_dtype) if need_h else None, None, gw, gb


class CosineEmbeddingNetwork(nn.Module):
    """IQN's cosine embedding (utils/net/discrete.py:124-155): a fraction in [0, 1] becomes
    relu(Linear(cos(pi i tau), i = 1..num_cosines)).  Module layout (``net.0``) as the
    reference's."""

    def __init__(self, num_cosines: int, embedding_dim: int) -> None:
        super().__init__()
        self.net = nn.Sequential(nn.Linear(num_cosines, embedding_dim), nn.ReLU())
        self.num_cosines = num_cosines
        self.embedding_dim = embedding_dim

    @staticmethod
    def cosines(taus: torch.Tensor, num_cosines: int) -> torch.Tensor:
        """discrete.py:147-152: cos(i pi tau), [b * N, num_cosines]."""
        batch_size, N = taus.shape[0], taus.shape[1]
        i_pi = np.pi * torch.arange(start=1, end=num_cosines + 1, dtype=taus.dtype,
                                    device=taus.device).view(1, 1, num_cosines)
        return torch.cos(taus.view(batch_size, N, 1) * i_pi).view(batch_size * N, num_cosines)

    def forward(self, taus: torch.Tensor) -> torch.Tensor:
        cosines = self.cosines(taus, self.num_cosines)
        return self.net(cosines).view(taus.shape[0], taus.shape[1], self.embedding_dim)

    def hadamard(self, h: torch.Tensor, taus: torch.Tensor, fused: bool = True) -> torch.Tensor:
        """(h.unsqueeze(1) * self(taus)).view(b * N, -1) (discrete.py:211-212): one launch each
        way on the GPU; the reference's torch lines on the CPU, with ``fused`` False and with
        more cosines than the kernel stages (_C.IQN_MAX_COSINES)."""
        lin = self.net[0]
        if fused and h.is_cuda and taus.is_cuda and h.dim() == 2 and \
                h.dtype == torch.float32 and taus.dtype == torch.float32 and \
                lin.weight.dtype == torch.float32 and self.num_cosines <= _C.IQN_MAX_COSINES:
            return _IQNEmbedFn.apply(h, taus, lin.weight, lin.bias)
        return (h.unsqueeze(1) * self(taus)).view(taus.shape[0] * taus.shape[1], -1)


class ImplicitQuantileNetwork(DiscreteCritic):
    """IQN's quantile Q-network (utils/net/discrete.py:158-214): constructor arguments,
    attributes and state_dict keys (``preprocess.*``, ``last.*``, ``embed_model.net.0.*``) as
    the reference's.  ``forward`` returns ((out, taus), hidden) with out the [b, A, N] view of
    the head's [b, N, A] output.  ``taus`` None draws them where the reference does (after the
    preprocess forward, one torch.rand), so a seeded CPU run consumes the reference's stream;
    IQNPolicy hands recorded or pre-drawn fractions in.  ``fused_embed = False``: the torch
    lines (``IQNPolicy.fused`` sets it on its networks)."""

    fused_embed = True

    def __init__(self, preprocess_net: nn.Module, action_shape, hidden_sizes: Sequence[int] = (),
                 num_cosines: int = 64, preprocess_net_output_dim: Optional[int] = None,
                 device="cpu") -> None:
        last_size = int(np.prod(action_shape))
        super().__init__(preprocess_net, hidden_sizes, last_size, preprocess_net_output_dim,
                         device)
        self.input_dim = getattr(preprocess_net, "output_dim", preprocess_net_output_dim)
        self.embed_model = CosineEmbeddingNetwork(num_cosines, self.input_dim).to(device)

    def forward(self, obs, sample_size: int, taus: Optional[torch.Tensor] = None,
                **kwargs: Any):
        logits, hidden = self.preprocess(obs, state=kwargs.get("state", None))
        batch_size = logits.size(0)
        if taus is None:
            taus = torch.rand(batch_size, sample_size, dtype=logits.dtype, device=logits.device)
        sample_size = taus.shape[1]
        embedding = self.embed_model.hadamard(logits, taus, self.fused_embed)
        out = self.last(embedding).view(batch_size, sample_size, -1).transpose(1, 2)
        return (out, taus), hidden


class _FQFProposeFn(torch.autograd.Function):
    """discrete.py:241-249 from the proposal logits [b, N] as one tsrl_fqf_propose_fwd launch:
    returns (taus [b, N + 1], tau_hats [b, N], entropies [b], logp [b, N]).  The backward is the
    analytic one for any incoming g_taus and g_entropies (cumsum, softmax, entropy); tau_hats are
    detached as in the reference and logp is the kernel's by-product for
    tsrl_fqf_fraction_loss_fwd_bwd."""

    @staticmethod
    def forward(ctx, logits):
        x = logits.detach().float().contiguous()
        if x.dim() != 2:
            raise ValueError(f"_FQFProposeFn: need [b, N] logits, got {tuple(x.shape)}")
        b, N = x.shape
        dev = x.device
        taus = torch.empty(b, N + 1, dtype=torch.float32, device=dev)
        tau_hats = torch.empty(b, N, dtype=torch.float32, device=dev)
        entropies = torch.empty(b, dtype=torch.float32, device=dev)
        logp = torch.empty(b, N, dtype=torch.float32, device=dev)
        _C.check(_C.lib().tsrl_fqf_propose_fwd(
            _C.ptr(x), b, N, _C.ptr(taus), _C.ptr(tau_hats), _C.ptr(entropies), _C.ptr(logp),
            _C.stream_ptr(dev)), "tsrl_fqf_propose_fwd")
        ctx.save_for_backward(logp, entropies)
        ctx.in_dtype = logits.dtype
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(tau_hats, logp)
        return taus, tau_hats, entropies, logp

    @staticmethod
    def backward(ctx, g_taus, g_hats, g_ent, g_logp):
        logp, entropies = ctx.saved_tensors
        # in f64 as the kernels' per-row arithmetic, rounded once: with one fraction near 1 the
        # softmax backward cancels (in f32 it missed the 4 x torch bound at N = 2)
        logp = logp.double()
        p = logp.exp()
        g = None
        if g_taus is not None:
            # taus[i] = sum_{k < i} p_k: dL/dp_k = sum_{i > k} g_taus[i], then the softmax
            g_p = g_taus[:, 1:].double().flip(1).cumsum(1).flip(1)
            g = p * (g_p - (p * g_p).sum(1, keepdim=True))
        if g_ent is not None:
            # dH/dl_k = -p_k (logp_k + H); a p_k of exactly 0 (logp -inf) contributes 0
            t = torch.where(p == 0, torch.zeros_like(p),
                            p * (logp + entropies.double().unsqueeze(1)))
            g_e = -g_ent.double().unsqueeze(1) * t
            g = g_e if g is None else g + g_e
        return None if g is None else g.to(ctx.in_dtype)


class FractionProposalNetwork(nn.Module):
    """FQF's fraction proposal network (utils/net/discrete.py:217-249): one Linear named ``net``
    with the reference's initialiser in its order, so a seeded CPU construction reproduces its
    weights.  ``forward`` returns (taus [b, N + 1], tau_hats [b, N], entropies [b]).  On a HIP
    device with f32 inputs and N <= _C.DIST_MAX_N the softmax, cumsum, pad, midpoints and
    entropy are one tsrl_fqf_propose_fwd launch (``_FQFProposeFn``) and the Linear's gradients
    come from ``_linear_grads``; elsewhere, and with ``fused = False`` (``FQFPolicy.fused``
    sets it), the reference's torch lines run."""

    fused = True

    def __init__(self, num_fractions: int, embedding_dim: int) -> None:
        super().__init__()
        self.net = nn.Linear(embedding_dim, num_fractions)
        torch.nn.init.xavier_uniform_(self.net.weight, gain=0.01)
        torch.nn.init.constant_(self.net.bias, 0)
        self.num_fractions = num_fractions
        self.embedding_dim = embedding_dim

    def takes_kernel(self, obs_embeddings: torch.Tensor) -> bool:
        return self.fused and obs_embeddings.is_cuda and obs_embeddings.dim() == 2 and \
            obs_embeddings.dtype == torch.float32 and self.net.weight.dtype == torch.float32 and \
            2 <= self.num_fractions <= _C.DIST_MAX_N

    def propose(self, obs_embeddings: torch.Tensor):
        """The kernel path with its by-products: (logits, taus, tau_hats, entropies, logp)."""
        logits = _LinearFn.apply(obs_embeddings, self.net.weight, self.net.bias)
        return (logits,) + _FQFProposeFn.apply(logits)

    def forward(self, obs_embeddings: torch.Tensor):
        if self.takes_kernel(obs_embeddings):
            return self.propose(obs_embeddings)[1:4]
        dist = torch.distributions.Categorical(logits=self.net(obs_embeddings))
        taus_1_N = torch.cumsum(dist.probs, dim=1)
        taus = torch.nn.functional.pad(taus_1_N, (1, 0))
        tau_hats = (taus[:, :-1] + taus[:, 1:]).detach() / 2.0
        entropies = dist.entropy()
        return taus, tau_hats, entropies


class FullQuantileFunction(ImplicitQuantileNetwork):
    """FQF's quantile network (utils/net/discrete.py:252-316): constructor arguments and
    state_dict keys are ImplicitQuantileNetwork's.  ``forward`` returns ((quantiles, fractions,
    quantiles_tau), hidden) with fractions = Batch(taus, tau_hats, entropies) proposed from the
    detached state embedding (or handed in), quantiles at tau_hats, and quantiles_tau, under
    no_grad and only while training, at taus[:, 1:-1].  ``want_quantiles_tau = False`` skips
    that second pass where nobody reads it (FQFPolicy's ``_target_q``)."""

    def _compute_quantiles(self, obs: torch.Tensor, taus: torch.Tensor) -> torch.Tensor:
        batch_size, sample_size = taus.shape
        embedding = self.embed_model.hadamard(obs, taus, self.fused_embed)
        return self.last(embedding).view(batch_size, sample_size, -1).transpose(1, 2)

    def forward(self, obs, propose_model: nn.Module, fractions=None,
                want_quantiles_tau: bool = True, **kwargs: Any):
        from tianshou_amd.data.batch import Batch
        logits, hidden = self.preprocess(obs, state=kwargs.get("state", None))
        if fractions is None:
            taus, tau_hats, entropies = propose_model(logits.detach())
            fractions = Batch(taus=taus, tau_hats=tau_hats, entropies=entropies)
        else:
            taus, tau_hats = fractions.taus, fractions.tau_hats
        quantiles = self._compute_quantiles(logits, tau_hats)
        quantiles_tau = None
        if self.training and want_quantiles_tau:
            with torch.no_grad():
                quantiles_tau = self._compute_quantiles(logits, taus[:, 1:-1])
        return (quantiles, fractions, quantiles_tau), hidden


class ActorCritic(nn.Module):
    """common.py:364-377."""

    def __init__(self, actor: nn.Module, critic: nn.Module) -> None:
        super().__init__()
        self.actor = actor
        self.critic = critic


def build_actor_critic_from_state(state: Dict[str, torch.Tensor], device="cpu"):
    """Rebuild get_actor_critic-shaped (Tanh MLP) actor/critic from a policy state_dict."""
    w0 = state["actor.preprocess_net.model.model.0.weight"]
    hidden = []
    i = 0
    while f"actor.preprocess_net.model.model.{i}.weight" in state:
        hidden.append(state[f"actor.preprocess_net.model.model.{i}.weight"].shape[0])
        i += 2
    obs_dim = w0.shape[1]
    act_dim = state["actor.mu.model.0.weight"].shape[0]
    from tianshou_amd.utils.models import get_actor_critic
    actor, critic = get_actor_critic((obs_dim,), hidden, (act_dim,), device)
    ac = ActorCritic(actor, critic)
    ac.load_state_dict({k: v for k, v in state.items()
                        if k.startswith("actor.") or k.startswith("critic.")}, strict=False)
    return actor.to(device), critic.to(device)
