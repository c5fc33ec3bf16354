"""Shared by tests/test_gpu_fvp.py: the Fisher-vector product of include/tsrl.h restated in f64
torch on the CPU, the reference's double-backward product (npg.py::_MVP) in a chosen dtype, and
the case table.  Flat vectors follow actor.parameters(): sigma_param, W1, b1, W2, b2, W3, b3."""
import torch

NAMES = ("sigma", "w1", "b1", "w2", "b2", "w3", "b3")
# (n, D, A, damping): one partial row / tile boundaries / more tiles than workgroups (257 CUs'
# worth of tiles + 1 row); padded pitch, K-chunk remainder, exact chunk, the resident panel,
# two panels (D > 384)
CASES = [(1, 3, 1, 0.1), (63, 33, 17, 0.0), (64, 64, 32, 0.1), (65, 3, 17, 0.1),
         (257, 376, 17, 0.1), (64 * 256 + 1, 33, 1, 0.0), (65, 376, 32, 0.0),
         (129, 420, 6, 0.1)]


def make(n, D, A, seed=0):
    """(params in flat order, X [n, D], v flat), all f64."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * k  # noqa: E731
    params = [r(A, 1, k=0.5), r(64, D, k=D ** -0.5), r(64, k=0.1), r(64, 64, k=0.125),
              r(64, k=0.1), r(A, 64, k=0.125), r(A, k=0.1)]
    return params, r(n, D), r(sum(p.numel() for p in params))


def split(flat, params):
    out, o = [], 0
    for p in params:
        out.append(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()
    return out


def fvp_f64(params, X, v, damping):
    ls, W1, b1, W2, b2, W3, b3 = params
    vs, V1, c1, V2, c2, V3, c3 = split(v, params)
    n = X.shape[0]
    h1 = torch.tanh(X @ W1.T + b1)
    h2 = torch.tanh(h1 @ W2.T + b2)
    Rh1 = (1 - h1 ** 2) * (X @ V1.T + c1)
    Rh2 = (1 - h2 ** 2) * (Rh1 @ W2.T + h1 @ V2.T + c2)
    g = (Rh2 @ W3.T + h2 @ V3.T + c3) * torch.exp(-2 * ls.view(-1)) / n
    dz2 = (g @ W3) * (1 - h2 ** 2)
    dz1 = (dz2 @ W2) * (1 - h1 ** 2)
    Fv = [2 * vs, dz1.T @ X, dz1.sum(0), dz2.T @ h1, dz2.sum(0), g.T @ h2, g.sum(0)]
    return torch.cat([t.reshape(-1) for t in Fv]) + damping * v


def autograd_mvp(params, X, v, damping, dtype):
    """npg.py::_MVP: the KL Hessian-vector product by double backward, in ``dtype``."""
    ps = [p.to(dtype).requires_grad_() for p in params]
    ls, W1, b1, W2, b2, W3, b3 = ps
    X, v = X.to(dtype), v.to(dtype)
    mu = torch.tanh(torch.tanh(X @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
    sd = (ls.view(1, -1) + torch.zeros_like(mu)).exp()
    new = torch.distributions.Independent(torch.distributions.Normal(mu, sd), 1)
    old = torch.distributions.Independent(torch.distributions.Normal(mu.detach(), sd.detach()), 1)
    kl = torch.distributions.kl_divergence(old, new).mean()
    gk = torch.cat([t.reshape(-1) for t in torch.autograd.grad(kl, ps, create_graph=True)])
    gg = torch.autograd.grad((gk * v).sum(), ps)
    return torch.cat([t.reshape(-1) for t in gg]).detach() + damping * v


def cg(mvp, b, nsteps=10, tol=1e-10):
    """npg.py::_conjugate_gradients; returns (x, iterations run, r.r after each)."""
    x, r, p = torch.zeros_like(b), b.clone(), b.clone()
    rdotr, hist = r.dot(r), []
    for i in range(nsteps):
        z = mvp(p)
        alpha = rdotr / p.dot(z)
        x += alpha * p
        r -= alpha * z
        new = r.dot(r)
        hist.append(float(new))
        if new < tol:
            break
        p = r + new / rdotr * p
        rdotr = new
    return x, i + 1, hist
