"""csrc/fvp.hip: the Fisher-vector product and the device CG of NPGPolicy / TRPOPolicy.

1. tsrl_fvp_prepare + tsrl_fvp_apply through the C ABI against the f64 restatement
   (tests/fvp_common.py).  Bound, per parameter block: max-abs and 2-norm error at most 4 x the
   same error of torch's f32 double backward on identical inputs (the reference's _MVP, on the
   CPU), floor 2^-23 ||F v||_2.  The 4 covers the other summation order (64-row tiles, one
   partial per workgroup) and 1 - h^2 formed from stored activations.
2. The device solve against a 10-step f64 CG, with and without the early stop.
3. NPGPolicy / TRPOPolicy.learn with fused_fvp on and off from one initial state.
Each test prints its measured ratios (profiles/fvp_gpu_tests.log)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from tests import fvp_common as fc
from tianshou_amd import _C

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Device:
    """One problem on the device: padded rows, the net descriptor, workspace, prepare done."""

    def __init__(self, params, X, dev):
        n, D = X.shape
        A = params[0].numel()
        self.P = sum(p.numel() for p in params)
        ldx = (D + 3) // 4 * 4
        self.x = torch.zeros(n, ldx, device=dev)
        self.x[:, :D] = X.float()
        self.w = [p.float().contiguous().to(dev) for p in params]
        offs = np.cumsum([0] + [p.numel() for p in params])[:7]
        sg, w1, b1, w2, b2, w3, b3 = (t.data_ptr() for t in self.w)
        self.net = _C.FvpNet(w1, b1, w2, b2, w3, b3, sg, *(int(o) for o in offs), self.P)
        self.nb = int(_C.lib().tsrl_fvp_workspace_bytes(n, D, A))
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device=dev)
        self.shape = (self.x.data_ptr(), ldx, n, D, A)
        _C.check(_C.lib().tsrl_fvp_prepare(*self.shape, ctypes.byref(self.net),
                                           self.ws.data_ptr(), self.nb, None), "prepare")

    def apply(self, v, out, damping, state=None):
        _C.check(_C.lib().tsrl_fvp_apply(
            *self.shape, ctypes.byref(self.net), v.data_ptr(), out.data_ptr(), damping,
            None if state is None else state.data_ptr(), self.ws.data_ptr(), self.nb, None),
            "apply")


def _ratios(got, ref32, ref64, params):
    """Worst (error of got) / max(error of ref32, floor / 4) over blocks and both norms."""
    floor = 2.0 ** -23 * float(ref64.norm())
    worst = 0.0
    for g, t, r in zip(fc.split(got, params), fc.split(ref32, params), fc.split(ref64, params)):
        for norm in (lambda d: float(d.abs().max()), lambda d: float(d.norm())):
            worst = max(worst, norm(g - r) / max(norm(t.double() - r), floor / 4))
    return worst


@pytest.mark.parametrize("n,D,A,damping", fc.CASES)
def test_product_matches_f64(dev, n, D, A, damping):
    params, X, v = fc.make(n, D, A)
    ref64 = fc.fvp_f64(params, X, v, damping)
    ref32 = fc.autograd_mvp(params, X, v, damping, torch.float32)
    d = _Device(params, X, dev)
    vd = v.float().to(dev)
    outs = []
    for _ in range(2):
        out = torch.full((d.P + 2 * GUARD,), float("nan"), device=dev)
        d.apply(vd, out[GUARD:], damping)
        assert out[:GUARD].isnan().all() and out[GUARD + d.P:].isnan().all()
        outs.append(out[GUARD:GUARD + d.P].cpu())
    assert torch.equal(outs[0], outs[1])
    worst = _ratios(outs[0].double(), ref32, ref64, params)
    print(f"fvp n={n} D={D} A={A} damping={damping}: worst error ratio to torch f32 {worst:.3f}")
    assert worst <= 4.0


def _solve(d, b, dev, damping=0.1):
    x, r, p, z = (torch.full((d.P,), float("nan"), device=dev) for _ in range(4))
    st = torch.empty(2, dtype=torch.float64, device=dev)
    L = _C.lib()
    _C.check(L.tsrl_cg_init(b.data_ptr(), d.P, *(t.data_ptr() for t in (x, r, p)),
                            st.data_ptr(), None), "cg_init")
    for _ in range(10):
        d.apply(p, z, damping, st)
        _C.check(L.tsrl_cg_step(*(t.data_ptr() for t in (x, r, p, z)), d.P, 1e-10,
                                st.data_ptr(), d.ws.data_ptr(), None), "cg_step")
    return x.cpu().double(), st.cpu()


@pytest.mark.parametrize("stop", (False, True))
def test_cg_matches_f64(dev, stop):
    params, X, b = fc.make(65, 33, 3, seed=1)
    mvp64 = lambda p: fc.fvp_f64(params, X, p, 0.1)  # noqa: E731
    if stop:
        # 12 power steps bring b close to the top eigenvector: the first CG step then cuts
        # r.r about 1500-fold; scaled so that r.r is 5e-12 after it (b.b about 8e-9)
        for _ in range(12):
            b = mvp64(b)
            b = b / b.norm()
        b = b * (5e-12 / fc.cg(mvp64, b.clone(), nsteps=1)[2][0]) ** 0.5
    x64, iters, hist = fc.cg(mvp64, b.clone())
    if stop:
        assert iters == 1 and float(b.dot(b)) >= 1e-9 and hist[0] * 10 <= 1e-10
        x10, _, _ = fc.cg(mvp64, b.clone(), tol=0.0)
    else:
        assert iters == 10 and min(hist) > 1e-9
    x32, _, _ = fc.cg(lambda p: fc.autograd_mvp(params, X, p, 0.1, torch.float32), b.float())
    x, st = _solve(_Device(params, X, dev), b.float().to(dev), dev)
    assert float(st[1]) == float(stop)
    floor = 2.0 ** -23 * float(x64.norm())
    for norm in (lambda t: float(t.abs().max()), lambda t: float(t.norm())):
        ratio = norm(x - x64) / max(norm(x32.double() - x64), floor / 4)
        print(f"cg stop={stop}: error ratio to torch f32 CG {ratio:.3f}")
        assert ratio <= 4.0
    if stop:
        assert float((x - x10).norm()) > 100 * float((x - x64).norm())


@pytest.mark.parametrize("tag", ("npg", "trpo"))
def test_learn_fused_matches_unfused(golden_dir, dev, tag, monkeypatch):
    from tests.test_npg import _policy
    from tianshou_amd.data import Batch
    z = np.load(os.path.join(golden_dir, "npg.npz"))
    D, A = int(z["D"]), int(z["A"])
    calls, L = [], _C.lib()
    monkeypatch.setattr(L, "tsrl_fvp_apply", (lambda f: lambda *a: (calls.append(1), f(*a))[1])(
        L.tsrl_fvp_apply))
    p = tag + "_"
    idx = z[p + "indices"]
    t = lambda a: torch.as_tensor(np.asarray(a), device=dev)  # noqa: E731
    runs = []
    for fused in (True, False):
        policy = _policy(z, tag, dev, D, A)
        policy._fused_fvp = fused
        batch = Batch(obs=t(z[p + "buf_obs"][idx]), act=t(z[p + "buf_act"][idx]).float(),
                      adv=t(z[p + "pf_adv"]), returns=t(z[p + "pf_returns"]),
                      v_s=t(z[p + "pf_v_s"]), logp_old=t(z[p + "pf_logp_old"]))
        np.random.seed(5)
        calls.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = policy.learn(batch, batch_size=len(idx) // 4, repeat=2)
        assert len(calls) == ((10 if tag == "npg" else 11) * 8 if fused else 0)
        runs.append((res, [q.detach().cpu().numpy() for q in policy.actor.parameters()]))
    (ra, pa), (rb, pb) = runs
    for k in rb:
        np.testing.assert_allclose(ra[k], rb[k], rtol=2e-3, atol=2e-4, err_msg=k)
    for a, b in zip(pa, pb):
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=2e-4)
