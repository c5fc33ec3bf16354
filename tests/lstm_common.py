"""Shared by tests/test_gpu_lstm.py and tests/test_lstm_host.py: ``lstm_last`` of include/tsrl.h
(csrc/lstm.hip) restated step by step in torch on the CPU (f64 reference, or f32: the reference
formulation's own error), its gradients by autograd, a seeded ``make`` and the case table.
Parameter lists follow nn.LSTM: per layer weight_ih, weight_hh, bias_ih, bias_hh."""
import torch

from tests.icm_common import split, worst_ratio  # noqa: F401

# (B, T, L, H, Din, initial state).  B: one partial tile / one row past a tile / several tiles
# with a ragged last one; Din: H, tiny, odd (K padding); every T, L, H with and without state
CASES = [(1, 1, 1, 64, 64, False), (33, 3, 2, 128, 128, True), (70, 3, 2, 64, 5, True),
         (33, 1, 2, 128, 17, False), (70, 1, 1, 128, 128, True), (1, 3, 2, 64, 17, True),
         (33, 3, 1, 128, 5, False), (70, 3, 2, 128, 17, True)]


def make(B, T, L, H, Din, with_state, seed=0):
    """(params, x [B, T, Din], h0, c0 [B, L, H] or None, d_out [B, H]) in f64."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k  # noqa: E731
    k, params = H ** -0.5, []
    for l in range(L):
        params += [r(4 * H, Din if l == 0 else H, k=k), r(4 * H, H, k=k), r(4 * H, k=k),
                   r(4 * H, k=k)]
    h0, c0 = (r(B, L, H), r(B, L, H)) if with_state else (None, None)
    return params, r(B, T, Din), h0, c0, r(B, H)


def lstm_last(params, x, h0=None, c0=None, dtype=torch.float64):
    """(hn, cn) [B, L, H] after the last step, gates i, f, g, o, computed in ``dtype``."""
    p, x = [t.to(dtype) for t in params], x.to(dtype)
    L, H, (B, T, _) = len(p) // 4, p[1].shape[1], x.shape
    h = [x.new_zeros(B, H) if h0 is None else h0[:, l].to(dtype) for l in range(L)]
    c = [x.new_zeros(B, H) if c0 is None else c0[:, l].to(dtype) for l in range(L)]
    for t in range(T):
        inp = x[:, t]
        for l in range(L):
            w_ih, w_hh, b_ih, b_hh = p[4 * l:4 * l + 4]
            i, f, g, o = (inp @ w_ih.T + b_ih + h[l] @ w_hh.T + b_hh).chunk(4, 1)
            c[l] = torch.sigmoid(f) * c[l] + torch.sigmoid(i) * torch.tanh(g)
            inp = h[l] = torch.sigmoid(o) * torch.tanh(c[l])
    return torch.stack(h, 1), torch.stack(c, 1)


def fwd_bwd(params, x, h0, c0, d_out, dtype=torch.float64):
    """(hn, cn, the parameter gradients flat, dx) for the seed d_out on hn[:, L - 1]."""
    p = [t.to(dtype).requires_grad_() for t in params]
    xx = x.to(dtype).requires_grad_()
    hn, cn = lstm_last(p, xx, h0, c0, dtype)
    *gp, dx = torch.autograd.grad(hn[:, -1], p + [xx], d_out.to(dtype))
    return hn.detach(), cn.detach(), torch.cat([t.reshape(-1) for t in gp]), dx
