"""The evaluation half of the fused actor/critic MLP (process_fn's v_s, v_s_ and logp_old),
entry point by entry point through the C ABI (include/tsrl.h), against float64 references
built from the same f32 inputs.

* tsrl_ppo_eval (csrc/mlp.hip eval_tail_kernel) on a CONSTRUCTED H1, placed in the fragment
  layout by mlp_common.rows_to_frag and so independent of the layer-1 kernels: layers 2-3, the
  value head and Independent(Normal(mu, exp(log_std)), 1).log_prob(act) in f64 from that H1.
* tsrl_ppo_eval_fused (csrc/mlp_x6.hip eval_ws_kernel + l1_ring_kernel<true, true>) against
  the whole graph from X[idx, :D] in f64.
* Bitwise properties that need no tolerance: values-only = the values of the log-prob run,
  position independence (what the V(s') shortcut of FusedEvalMixin._eval_values rests on),
  gather = copy, padded pitch = packed pitch, the fragment buffer's pad rows.
* Every refusal of both entry points, and the host paths around them (the chunk loop of
  FusedActorCritic.evaluate, the V(s') shortcut).

Error measure, per ROW (one bad row cannot hide behind the tensor's largest magnitude):
e_i = |got_i - ref_i| / S_i, for the value S_i = |b3c| + sum_k |w3c_k h2_ik|, for the log-prob
S_i = sum_a (d_ia^2 / (2 sigma_a^2) + |log sigma_a| + log sqrt(2 pi)), both from the f64
reference.  Bound: max_i e_i <= max(4 x the same quantity of torch's own f32 GPU arithmetic on
the same graph, EVAL_FLOOR).  Every input table has NaN in the rows idx does not name and in
its pad columns, every workspace and output starts as NaN, every output ends in a canary.
"""
import functools
import math

import pytest
import torch

from tests.mlp_common import _nets, gauss_dist, rows_to_frag
from tests.test_gpu_mlp_bwd import NAN, _bits, _canary_ok, _l1_frag, _last_error, _out

pytestmark = pytest.mark.gpu

H = 64
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)

# EVAL_FLOOR: per entry point and output, the largest e (above) of torch f32 -- the same graph
# in f32 on the GPU -- over EVAL_CASES + EVAL_BIG (tsrl_ppo_eval) and FUSED_CASES + FUSED_BIG
# (tsrl_ppo_eval_fused), measured on an MI355X and rounded up to two digits.  It covers the
# cases where torch's own error is 0 or tiny (n = 1).  Next to each: the largest e of the kernel
# and of torch f32 over those cases (the torch maxima sit at n = 131105, at the directed n =
# 1000, A = 1 case with log_std = -3, at n = 262401 and at the saturating case).  No case needed
# a wider bound: the closest comes to 0.44 of its own.
EVAL_FLOOR = {
    "eval.value": 2.2e-07,   # kernel 1.386e-07, torch f32 2.156e-07
    "eval.logp": 3.6e-06,    # kernel 5.246e-06, torch f32 3.529e-06
    "fused.value": 3.2e-07,  # kernel 4.156e-07, torch f32 3.140e-07
    "fused.logp": 4.9e-07,   # kernel 4.143e-07, torch f32 4.840e-07
}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _dev():
    return torch.device("cuda", 0)


# =============================================================================================
# Shared: weights, references, the two entry points, the check
# =============================================================================================
def _tail_weights(g, A):
    """Layers 2-3 of both nets and log_std, scaled as test_gpu_mlp_bwd._tail_case."""
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g))  # noqa: E731
    return {"w2a": r(H, H, k=0.15), "b2a": r(H, k=0.1), "w2c": r(H, H, k=0.15), "b2c": r(H, k=0.1),
            "w3a": r(A, H, k=0.15), "b3a": r(A, k=0.1), "w3c": r(1, H, k=0.15), "b3c": r(1, k=0.1),
            "sigma": r(A, k=0.3) - 0.5}


def _l1_weights(g, D):
    """Layer 1 of both nets as _tail_case at D = 8 (0.4, 0.2), the weights scaled by
    sqrt(8 / D) so that the pre-activations keep their size at every width."""
    k = 0.4 * math.sqrt(8.0 / D)
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g))  # noqa: E731
    return {"w1a": r(H, D, k=k), "b1a": r(H, k=0.2), "w1c": r(H, D, k=k), "b1c": r(H, k=0.2)}


def _graph(inp, P, act, from_x):
    """The evaluation forward on H1 [n, 128] or, from_x, on the observation rows [n, D]."""
    if from_x:
        inp = torch.cat([torch.tanh(inp @ P["w1a"].T + P["b1a"]),
                         torch.tanh(inp @ P["w1c"].T + P["b1c"])], 1)
    mu = torch.tanh(inp[:, :H] @ P["w2a"].T + P["b2a"]) @ P["w3a"].T + P["b3a"]
    h2c = torch.tanh(inp[:, H:] @ P["w2c"].T + P["b2c"])
    value = (h2c @ P["w3c"].T + P["b3c"]).flatten()
    logp = gauss_dist(mu, P["sigma"]).log_prob(act)
    return value, logp, mu, h2c


def _reference(inp, W, act, from_x, ref_device):
    """(f64 reference with the per-row scales S, torch f32 on the GPU) of one case."""
    with torch.no_grad():
        P = {k: v.to(ref_device, torch.float64) for k, v in W.items()}
        a64 = act.to(ref_device, torch.float64)
        value, logp, mu, h2c = _graph(inp.to(ref_device, torch.float64), P, a64, from_x)
        sig = P["sigma"].exp()
        d = a64 - mu
        ref = {"value": value, "logp": logp,
               "S_value": P["b3c"].abs() + (h2c.abs() * P["w3c"].abs()).sum(1),
               "S_logp": (d * d / (2.0 * sig * sig) + P["sigma"].abs() + LOG_SQRT_2PI).sum(1)}
        P32 = {k: v.to(_dev(), torch.float32) for k, v in W.items()}
        v32, l32, _, _ = _graph(inp.to(_dev(), torch.float32), P32, act.to(_dev()), from_x)
    return ref, {"value": v32, "logp": l32}


def _tw(W, actor=True):
    from tianshou_amd import _C
    a = (lambda k: _C.ptr(W[k])) if actor else (lambda k: None)
    return _C.TailWeights(a("w2a"), a("b2a"), _C.ptr(W["w2c"]), _C.ptr(W["b2c"]), a("w3a"),
                          a("b3a"), _C.ptr(W["w3c"]), _C.ptr(W["b3c"]), a("sigma"))


def _finish(v, lp, n, logp):
    """Canaries behind both outputs; nothing written to a log-prob buffer that was not
    handed over."""
    assert _canary_ok(v, n), "written past value_out[n]"
    assert _canary_ok(lp, n), "written past logp_out[n]"
    if not logp:
        assert bool(torch.isnan(lp[:n]).all()), "logp buffer written although logp_out is NULL"
    return v[:n], (lp[:n] if logp else None)


def _run_eval(frag, n, W, A, act, logp=True, actor=True):
    """tsrl_ppo_eval into fresh NaN-filled outputs.  logp False: logp_out = act = NULL;
    actor False: the actor's pointers of tsrl_tail_weights NULL."""
    from tianshou_amd import _C
    dev = _dev()
    L, s = _C.lib(), _C.stream_ptr(dev)
    v, lp = _out(n, dev), _out(n, dev)
    tw = _tw(W, actor)
    _C.check(L.tsrl_ppo_eval(_C.ptr(frag), n, tw, A, _C.ptr(act) if logp else None, _C.ptr(v),
                             _C.ptr(lp) if logp else None, s), "tsrl_ppo_eval")
    torch.cuda.synchronize()
    return _finish(v, lp, n, logp)


@functools.lru_cache(maxsize=None)
def _fused_ws_bytes():
    from tianshou_amd import _C
    return int(_C.lib().tsrl_ppo_eval_fused_workspace_bytes())


def _split_w(W1, D):
    """tsrl_mlp_split_w into a NaN-filled buffer."""
    from tianshou_amd import _C
    dev = _dev()
    L, s = _C.lib(), _C.stream_ptr(dev)
    ws = torch.full(((int(L.tsrl_mlp_split_bytes(D)) + 3) // 4,), NAN, device=dev)
    _C.check(L.tsrl_mlp_split_w(_C.ptr(W1["w1a"]), _C.ptr(W1["w1c"]), D, _C.ptr(ws), s),
             "tsrl_mlp_split_w")
    return ws


def _run_fused(X, ldx, idx, n, D, W1, W, A, act, logp=True, actor=True):
    """tsrl_ppo_eval_fused into fresh NaN-filled outputs and a fresh NaN-filled workspace with
    a canary of its own."""
    from tianshou_amd import _C
    dev = _dev()
    L, s = _C.lib(), _C.stream_ptr(dev)
    wsplit = _split_w(W1, D)
    nb = _fused_ws_bytes()
    assert nb % 4 == 0
    evw = _out(nb // 4, dev)
    v, lp = _out(n, dev), _out(n, dev)
    tw = _tw(W, actor)
    _C.check(L.tsrl_ppo_eval_fused(_C.ptr(X), ldx, _C.ptr(idx), n, D, _C.ptr(wsplit),
                                   _C.ptr(W1["b1a"]), _C.ptr(W1["b1c"]), tw, A,
                                   _C.ptr(act) if logp else None, _C.ptr(v),
                                   _C.ptr(lp) if logp else None, _C.ptr(evw), nb, s),
             "tsrl_ppo_eval_fused")
    torch.cuda.synchronize()
    assert _canary_ok(evw, nb // 4), "written past the evaluation workspace"
    return _finish(v, lp, n, logp)


def _row_err(got, ref, S):
    e = (got.to(ref.device).double() - ref).abs() / S
    i = int(e.argmax())
    return float(e[i]), i


def _check(kind, tag, got, ref, t32):
    """Both outputs of one run, every live row, against the case's f64 reference: finite, and
    the largest per-row e within max(4 x torch f32's, EVAL_FLOOR); prints both figures and
    names the case and the row of the largest e on failure."""
    bad = []
    for out in ("value", "logp"):
        assert got[out].shape == ref[out].shape, (out, got[out].shape)
        assert bool(torch.isfinite(got[out]).all()), f"{kind} {tag}: {out} not finite"
        ek, ik = _row_err(got[out], ref[out], ref["S_" + out])
        et, _ = _row_err(t32[out], ref[out], ref["S_" + out])
        floor = EVAL_FLOOR[f"{kind}.{out}"]
        print(f"EVAL {kind}.{out} {tag}: e_kernel {ek:.4g} e_torch_f32 {et:.4g} (row {ik})")
        if not ek <= max(4.0 * et, floor):
            bad.append(f"{out}: e_kernel {ek:.3g} > max(4 x {et:.3g}, {floor:.3g}) at row {ik}: "
                       f"got {float(got[out][ik])!r}, f64 {float(ref[out][ik])!r}")
    assert not bad, f"{kind} {tag}: " + "; ".join(bad)


# =============================================================================================
# 1. tsrl_ppo_eval on a constructed H1
# =============================================================================================
EVAL_NS = (1, 31, 32, 33, 127, 128, 129, 1000)
EVAL_AS = (1, 4, 5, 8, 16, 17, 31, 32)
# n = 1000, A in {1, 17, 32}: the directed rows (directed = 1; at A = 1, where one log_std entry
# cannot be both, 1 puts it at -3 and 2 at +1)
DIRECTED_AS = (1, 17, 32)


def _eval_cases():
    cases = [(n, A, 0) for n in EVAL_NS for A in (6, 17)]
    for A in EVAL_AS:
        for n in (33, 1000):
            if (n, A, 0) not in cases:
                cases.append((n, A, 0))
    cases = [(n, A, int(n == 1000 and A in DIRECTED_AS)) for n, A, _ in cases]
    cases.append((1000, 1, 2))
    return cases


EVAL_CASES = _eval_cases()
# past 1024 workgroups x 4 waves x 32 rows = 131072 rows: the second grid-stride pass of
# eval_tail_kernel, whose prefetch of the next actor tile sits under `bt + bstep < ntiles`
EVAL_BIG = (131072 + 33, 17)


def _kernel_mu_row(frag, n, W, A, mu_hat, row):
    """The mean of one row exactly as eval_tail_kernel computes it, fl(mu + b3a), from runs of
    the kernel itself: with log_std[a] = -40 (sigma^2 = 1.8e-35) and the other entries 0 the
    log-prob of the row is 40 - A log sqrt(2 pi) when act[a] equals that mean to the bit, and
    lower by (act[a] - mean)^2 / (2 sigma^2) >= 1e12 otherwise; that excess gives |act[a] -
    mean| to 1e-7 relative, far finer than the spacing of the floats there, and a second run
    tells the sign.  A last run with every log_std at -40 confirms all A entries at once."""
    import numpy as np
    dev = _dev()
    act = mu_hat.to(dev).clone()
    base = 40.0 - A * LOG_SQRT_2PI
    out = torch.empty(A)
    for a in range(A):
        ls = torch.zeros(A)
        ls[a] = -40.0
        Wp = dict(W, sigma=ls.to(dev))
        sig = torch.exp(Wp["sigma"][a:a + 1])
        var2 = 2.0 * float(sig * sig)

        def excess(t):
            act[row, a] = float(t)
            return base - float(_run_eval(frag, n, Wp, A, act)[1][row])

        m0 = float(mu_hat[row, a])
        found = None
        x = excess(m0)
        if x < 1.0:
            found = np.float32(m0)
        else:
            dist = math.sqrt(x * var2)
            for cand in (np.float32(m0 + dist), np.float32(m0 - dist)):
                if excess(cand) < 1.0:
                    found = cand
                    break
        assert found is not None, f"no action with a zero difference for row {row}, action {a}"
        act[row, a] = float(found)
        out[a] = float(found)
    Wp = dict(W, sigma=torch.full((A,), -40.0, device=dev))
    lp = float(_run_eval(frag, n, Wp, A, act)[1][row])
    assert abs(lp - A * (40.0 - LOG_SQRT_2PI)) < 1.0, lp
    return out


@functools.lru_cache(maxsize=None)
def _eval_case(n, A, directed=0):
    """One tsrl_ppo_eval case on the device with its f64 CPU reference and torch's f32 GPU run;
    computed once and shared (nothing in it is written afterwards)."""
    dev = _dev()
    g = torch.Generator().manual_seed(104729 * n + 211 * A + directed)
    H1 = torch.tanh(2.0 * torch.rand(n, 128, generator=g) - 1.0)
    W = _tail_weights(g, A)
    eps = torch.randn(n, A, generator=g)
    if directed:
        H1[3], H1[4] = 1.0, -1.0              # layer-2 pre-activations at their largest
        if directed == 2:
            W["sigma"][0] = 1.0
        else:
            W["sigma"][0] = -3.0
            if A > 1:
                W["sigma"][A - 1] = 1.0
        sign = torch.where(torch.arange(A) % 2 == 0, 1.0, -1.0)
        eps[1], eps[2] = 10.0 * sign, -100.0 * sign   # actions 10 and 100 sigma from mu
    Wd = {k: v.to(dev) for k, v in W.items()}
    frag = rows_to_frag(H1, NAN).to(dev)      # pad rows NaN (test_eval_pad_rows_are_free)
    with torch.no_grad():
        mu = torch.tanh(H1[:, :H] @ W["w2a"].T + W["b2a"]) @ W["w3a"].T + W["b3a"]
    act = mu + W["sigma"].exp() * eps         # stored rollout-style
    if directed:
        act[0] = _kernel_mu_row(frag, n, Wd, A, mu, 0)
    ref, t32 = _reference(H1, W, act, False, "cpu")
    return dict(n=n, A=A, frag=frag, H1=H1, W=Wd, act=act.to(dev), ref=ref, t32=t32)


@pytest.mark.parametrize("n,A,directed", EVAL_CASES)
def test_eval_matches_f64(dev, n, A, directed):
    """tsrl_ppo_eval on H1 = tanh(U(-1, 1)) placed by rows_to_frag (pad rows NaN), log_std =
    0.3 N(0, 1) - 0.5, actions mu + sigma eps: value and log-prob of every row within the
    bound of the module docstring.  Rows 1..33 and 127..129 leave dead lanes in the 32-row wave
    tiles and dead waves in the 128-row workgroups; A = 1..32 walks the lane-to-action map a =
    rho(r) + 4 h over the 32-row mu-head image with zero rows past A.  directed: row 0 acts
    exactly at the kernel's own mean (_kernel_mu_row), rows 1 and 2 act 10 and 100 sigma away,
    rows 3 and 4 have H1 = +1 and -1 throughout, log_std holds -3 and +1."""
    case = _eval_case(n, A, directed)
    v, lp = _run_eval(case["frag"], n, case["W"], A, case["act"])
    _check("eval", f"n={n} A={A} directed={directed}", {"value": v, "logp": lp}, case["ref"],
           case["t32"])


def test_eval_second_grid_stride_pass(dev):
    """n = 131072 + 33, A = 17: the grid is capped at 1024 workgroups of 4 row tiles, so the
    first two workgroups take a second pass (the last tile with one live row) and every other
    wave must NOT prefetch past the buffer.  H1 from tsrl_mlp_l1_fwd_x6 at D = 8, read back with
    frag_to_rows_dev; the f64 reference on the GPU."""
    from tests.test_gpu_mlp import frag_to_rows_dev
    n, A = EVAL_BIG
    D = 8
    g = torch.Generator().manual_seed(n)
    W1 = {k: v.to(dev) for k, v in _l1_weights(g, D).items()}
    W = _tail_weights(g, A)
    X = torch.randn(n, D, generator=g).to(dev)
    frag = _l1_frag(dev, "x6", X, D, None, n, D, W1["w1a"], W1["b1a"], W1["w1c"], W1["b1c"])
    H1 = frag_to_rows_dev(frag, n)
    assert bool(torch.isfinite(H1).all())
    Wd = {k: v.to(dev) for k, v in W.items()}
    with torch.no_grad():
        mu = torch.tanh(H1[:, :H] @ Wd["w2a"].T + Wd["b2a"]) @ Wd["w3a"].T + Wd["b3a"]
        act = mu + Wd["sigma"].exp() * torch.randn(n, A, generator=g).to(dev)
    ref, t32 = _reference(H1, W, act, False, dev)
    v, lp = _run_eval(frag, n, Wd, A, act)
    _check("eval", f"n={n} A={A} directed=0", {"value": v, "logp": lp}, ref, t32)


# =============================================================================================
# 2. tsrl_ppo_eval_fused from X
# =============================================================================================
_MODES = ("none", "perm", "rep")
FUSED_NS = (1, 31, 32, 33, 255, 256, 257, 1000)


def _fused_cases():
    # every row count of the 32-row wave tiles and the 256-row ring tiles, all three index modes
    cases = [(n, 8, 8, A, m, "std") for n in FUSED_NS for A in (6, 17) for m in _MODES]
    # widths: one 32-column chunk partly filled; exactly one; two with the last almost wholly
    # past dq = roundup(D, 4); the headline width -- then the padded pitches
    for i, (D, ldx) in enumerate(((32, 32), (36, 36), (376, 376), (376, 384), (36, 44))):
        cases.append((257, D, ldx, 6, _MODES[i % 3], "std"))
        cases.append((1000, D, ldx, 17, _MODES[(i + 1) % 3], "std"))
    cases.append((257, 36, 44, 6, "perm", "sat"))   # X scaled by 50: layer 1 saturates
    return cases


FUSED_CASES = _fused_cases()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _fused_big():
    """(n, what): tpw = ntiles / CUs tiles of 256 rows per workgroup."""
    c = _cus()
    return ((2 * 256 * c + 33, "tpw = 2, a ragged last tile in a workgroup of one tile"),
            (4 * 256 * c + 257, "tpw = 4, a last workgroup of two tiles, the second with 1 row"))


@functools.lru_cache(maxsize=None)
def _fused_case(n, D, ldx, A, mode, kind):
    """One tsrl_ppo_eval_fused case: X [N, ldx] with NaN in the rows idx does not name and in
    the columns roundup(D, 4)..ldx, the f64 reference (CPU to 4096 rows, GPU above) and torch
    f32 on the GPU from X[idx, :D]."""
    dev = _dev()
    assert D % 4 == 0   # columns D..roundup(D, 4) must be zeros: FusedActorCritic.rows' job
    g = torch.Generator().manual_seed(15485863 * n + 7919 * D + 31 * ldx + 3 * A
                                      + _MODES.index(mode))
    if mode == "none":
        N, idx = n, None
    elif mode == "perm":
        N = n + 29
        idx = torch.randperm(N, generator=g)[:n]
    else:
        N = n // 2 + 5
        idx = torch.randint(0, N, (n,), generator=g)
    x = torch.randn(N, D, generator=g) * (50.0 if kind == "sat" else 1.0)
    X = torch.full((N, ldx), NAN)
    X[:, :D] = x
    if idx is not None:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        X[dead] = NAN
    W1, W = _l1_weights(g, D), _tail_weights(g, A)
    xi = x if idx is None else x[idx]
    assert bool(torch.isfinite(xi).all())
    eps = torch.randn(n, A, generator=g)
    rdev = "cpu" if n <= 4096 else dev
    P = {k: v.to(rdev) for k, v in {**W1, **W}.items()}
    with torch.no_grad():
        mu = _graph(xi.to(rdev), P, torch.zeros(n, A, device=rdev), True)[2]
        act = mu + P["sigma"].exp() * eps.to(rdev)
    ref, t32 = _reference(xi, {**W1, **W}, act, True, rdev)
    return dict(n=n, D=D, ldx=ldx, A=A, X=X.to(dev), xi=xi,
                idx=None if idx is None else idx.to(dev),
                W1={k: v.to(dev) for k, v in W1.items()}, W={k: v.to(dev) for k, v in W.items()},
                act=act.to(dev), ref=ref, t32=t32)


def _run_fused_case(case, **kw):
    return _run_fused(case["X"], case["ldx"], case["idx"], case["n"], case["D"], case["W1"],
                      case["W"], case["A"], case["act"], **kw)


@pytest.mark.parametrize("n,D,ldx,A,mode,kind", FUSED_CASES)
def test_fused_eval_matches_f64(dev, n, D, ldx, A, mode, kind):
    """tsrl_ppo_eval_fused against the whole graph from X[idx, :D] in f64, layer-1 weights
    split by tsrl_mlp_split_w into a NaN-filled buffer: bound as the module docstring.  Index
    modes: none; a permutation into n + 29 rows; duplicates.  Row counts 255..257 end and start
    a 256-row ring tile.  Padded pitches (384 for 376, 44 for 36) carry NaN in the columns the
    kernel's comment says are never read."""
    case = _fused_case(n, D, ldx, A, mode, kind)
    v, lp = _run_fused_case(case)
    _check("fused", f"n={n} D={D} ldx={ldx} A={A} {mode} {kind}", {"value": v, "logp": lp},
           case["ref"], case["t32"])


@pytest.mark.parametrize("which", [0, 1])
def test_fused_eval_tiles_per_workgroup(dev, which):
    """n = 2 x 256 x CUs + 33 (tpw = 2) and 4 x 256 x CUs + 257 (tpw = 4, the last workgroup
    with fewer tiles than the others), D = 8, A = 17, a permutation idx on the second; f64 on
    the GPU."""
    n, what = _fused_big()[which]
    case = _fused_case(n, 8, 8, 17, _MODES[which], "std")
    v, lp = _run_fused_case(case)
    _check("fused", f"n={n} D=8 ldx=8 A=17 {_MODES[which]} big ({what})",
           {"value": v, "logp": lp}, case["ref"], case["t32"])


def _policy(dev, D, A, seed):
    from tianshou_amd.env import Box
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.models import fixed_std_normal
    actor, critic = _nets(D, A, dev, seed)
    optim = torch.optim.Adam(list(actor.parameters()) + list(critic.parameters()), lr=1e-4)
    pol = PPOPolicy(actor, critic, optim, fixed_std_normal, action_space=Box(-1.0, 1.0, (A,)),
                    fused_mlp=True)
    assert pol._mlp is not None
    return pol


def _layer_weights(mlp):
    Ls = mlp.L
    W = {}
    for k in ("1a", "1c", "2a", "2c", "3a", "3c"):
        W["w" + k] = Ls["w" + k].weight.detach().cpu()
        W["b" + k] = Ls["w" + k].bias.detach().cpu()
    W["sigma"] = Ls["sigma"].detach().cpu().flatten()
    return W


@pytest.mark.parametrize("mode", ["none", "perm"])
@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_unaligned_width_matches_f64(dev, monkeypatch, mode, fused):
    """D = 17 through FusedActorCritic.evaluate: rows of 17 floats are neither 16-byte aligned
    nor a multiple of 4 apart, so FusedActorCritic.rows hands the kernels its zero-padded
    [n, 20] copy; the reference reads obs[idx, :17] and the layers' own weights.  Both forms
    of evaluate (tsrl_ppo_eval_fused; tsrl_mlp_l1_fwd_x6 + tsrl_ppo_eval) meet the bound of
    the graph from X, n = 257, A = 6."""
    import tianshou_amd.policy.fused_mlp as fm
    monkeypatch.setattr(fm, "EVAL_FUSED", fused)
    D, A, n = 17, 6, 257
    mlp = _policy(dev, D, A, 31)._mlp
    W = _layer_weights(mlp)
    g = torch.Generator().manual_seed(17)
    N = n if mode == "none" else n + 29
    idx = None if mode == "none" else torch.randperm(N, generator=g)[:n]
    x = torch.randn(N, D, generator=g)
    obs = x.clone()
    if idx is not None:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        obs[dead] = NAN
    xi = x if idx is None else x[idx]
    with torch.no_grad():
        mu = _graph(xi, W, torch.zeros(n, A), True)[2]
        act = mu + W["sigma"].exp() * torch.randn(n, A, generator=g)
    ref, t32 = _reference(xi, W, act, True, "cpu")
    v, lp = mlp.evaluate(obs.to(dev), act.to(dev), None if idx is None else idx.to(dev))
    torch.cuda.synchronize()
    _check("fused", f"n={n} D=17 A={A} {mode} evaluate(EVAL_FUSED={fused})",
           {"value": v, "logp": lp}, ref, t32)


# =============================================================================================
# 3. Bitwise properties
# =============================================================================================
@pytest.mark.parametrize("n", [33, 257])
def test_eval_values_only_bitwise(dev, n):
    """3a, tsrl_ppo_eval: logp_out = act = NULL, the actor's pointers of tsrl_tail_weights NULL
    and the actor's feature tiles of the fragment buffer NaN: the value bits of the log-prob
    run, and nothing written to a log-prob buffer."""
    case = _eval_case(n, 6)
    v, _ = _run_eval(case["frag"], n, case["W"], 6, case["act"])
    assert bool(torch.isfinite(v).all())
    v1, none = _run_eval(case["frag"], n, case["W"], 6, None, logp=False)
    assert none is None and torch.equal(_bits(v), _bits(v1))
    crit = case["frag"].clone()
    crit.view(-1, 4, 1024)[:, :2] = NAN        # feature tiles 0, 1: the actor's 64 features
    v2, _ = _run_eval(crit, n, case["W"], 6, None, logp=False, actor=False)
    assert torch.equal(_bits(v), _bits(v2))


@pytest.mark.parametrize("n", [33, 257])
def test_fused_eval_values_only_bitwise(dev, n):
    """3a, tsrl_ppo_eval_fused: logp_out = act = NULL, with and without the actor's pointers:
    the value bits of the log-prob run (EvalArgs.w2a then aliases w2c and eval_ws_kernel takes
    null actor pointers)."""
    case = _fused_case(n, 8, 8, 6, "perm", "std")
    v, _ = _run_fused_case(case)
    assert bool(torch.isfinite(v).all())
    v1, none = _run_fused_case(case, logp=False)
    assert none is None and torch.equal(_bits(v), _bits(v1))
    v2, _ = _run_fused_case(case, logp=False, actor=False)
    assert torch.equal(_bits(v), _bits(v2))


POS_N = 2 * 256 + 33


def test_eval_position_independent(dev):
    """3b, tsrl_ppo_eval: one H1 row and one action replicated 545 times give one bit pattern
    in every position of both outputs, the one of an n = 1 call."""
    case = _eval_case(33, 17)
    h, a = case["H1"][7:8], case["act"][7:8]
    v1, l1 = _run_eval(rows_to_frag(h, NAN).to(dev), 1, case["W"], 17, a.contiguous())
    frag = rows_to_frag(h.repeat(POS_N, 1), NAN).to(dev)
    v, lp = _run_eval(frag, POS_N, case["W"], 17, a.repeat(POS_N, 1).contiguous())
    assert bool(torch.isfinite(v1).all() and torch.isfinite(l1).all())
    assert bool((_bits(v) == _bits(v1)).all()) and bool((_bits(lp) == _bits(l1)).all())


@pytest.mark.parametrize("use_idx", [False, True])
def test_fused_eval_position_independent(dev, use_idx):
    """3b, tsrl_ppo_eval_fused: one observation row and one action replicated 545 times (as 545
    copies, or as idx naming one row of a table whose other rows are NaN) give one bit pattern
    in every output position, the one of an n = 1 call."""
    case = _fused_case(33, 36, 36, 17, "none", "std")
    D, A, W1, W = 36, 17, case["W1"], case["W"]
    x, a = case["X"][5:6].contiguous(), case["act"][5:6].contiguous()
    v1, l1 = _run_fused(x, D, None, 1, D, W1, W, A, a)
    if use_idx:
        X = torch.full((3, D), NAN, device=dev)
        X[1] = x[0]
        idx = torch.ones(POS_N, dtype=torch.int64, device=dev)
    else:
        X, idx = x.repeat(POS_N, 1).contiguous(), None
    v, lp = _run_fused(X, D, idx, POS_N, D, W1, W, A, a.repeat(POS_N, 1).contiguous())
    assert bool(torch.isfinite(v1).all() and torch.isfinite(l1).all())
    assert bool((_bits(v) == _bits(v1)).all()) and bool((_bits(lp) == _bits(l1)).all())


@pytest.mark.parametrize("n,D,pad", [(257, 36, 44), (1000, 376, 384)])
def test_fused_eval_gather_equals_copy(dev, n, D, pad):
    """3c: idx into a table (unnamed rows NaN) gives the bits of the same rows copied
    contiguously with idx = NULL, and a padded pitch (NaN pads) the bits of the packed one."""
    case = _fused_case(n, D, pad, 6 if n == 257 else 17, "perm" if n == 257 else "rep", "std")
    A, W1, W, act = case["A"], case["W1"], case["W"], case["act"]
    v, lp = _run_fused_case(case)                                  # gathered, padded pitch
    packed = case["X"][:, :D].contiguous()
    vp, lpp = _run_fused(packed, D, case["idx"], n, D, W1, W, A, act)  # gathered, packed
    rows = case["X"][case["idx"]].contiguous()
    vc, lpc = _run_fused(rows, pad, None, n, D, W1, W, A, act)     # copied, padded pitch
    assert bool(torch.isfinite(v).all() and torch.isfinite(lp).all())
    for what, a, b in (("pitch", vp, lpp), ("copy", vc, lpc)):
        assert torch.equal(_bits(v), _bits(a)), what
        assert torch.equal(_bits(lp), _bits(b)), what


@pytest.mark.parametrize("n", [33, 129, 1000])
def test_eval_pad_rows_are_free(dev, n):
    """3d: the outputs of tsrl_ppo_eval for the rows < n keep every bit whether the rows n.. of
    the last 32-row tile (and of the last 128-row block) hold NaN, Inf or finite values: unlike
    tsrl_ppo_tail_stage this kernel has no pad-row requirement (include/tsrl.h)."""
    case = _eval_case(n, 6)
    res = []
    for fill in (NAN, float("inf"), 0.625):
        frag = rows_to_frag(case["H1"], fill).to(dev)
        res.append(_run_eval(frag, n, case["W"], 6, case["act"]))
    assert bool(torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][1]).all())
    for v, lp in res[1:]:
        assert torch.equal(_bits(v), _bits(res[0][0]))
        assert torch.equal(_bits(lp), _bits(res[0][1]))


# =============================================================================================
# 4. Refusals
# =============================================================================================
def _untouched(*outs):
    torch.cuda.synchronize()
    for t, m in outs:
        assert bool(torch.isnan(t[:m]).all()) and _canary_ok(t, m)


def test_eval_refusals(dev):
    """tsrl_ppo_eval returns non-zero, names itself in tsrl_last_error and leaves the NaN-filled
    outputs alone for: act_dim 0 and 33, logp_out without act, a fragment pointer 4 bytes off
    16-byte alignment, a NULL critic weight, a NULL actor weight with logp_out; n = 0 returns
    0 and writes nothing.  Every one of these returns before a launch."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    n, A = 33, 6
    case = _eval_case(n, A)
    W, frag, act = case["W"], case["frag"], case["act"]
    v, lp = _out(n, dev), _out(n, dev)
    shifted = torch.full((frag.numel() + 4,), 0.5, device=dev)[1:]
    assert shifted.data_ptr() % 16 == 4

    def call(frag_=frag, n_=n, W_=W, A_=A, act_=act, lp_=lp, actor=True):
        tw = _tw(W_, actor)
        return L.tsrl_ppo_eval(_C.ptr(frag_), n_, tw, A_, _C.ptr(act_), _C.ptr(v), _C.ptr(lp_), s)

    bad = {"act_dim 0": dict(A_=0), "act_dim 33": dict(A_=33),
           "logp_out without act": dict(act_=None),
           "h1frag off alignment": dict(frag_=shifted),
           "null actor weights with logp_out": dict(actor=False)}
    for k in ("w2c", "b2c", "w3c", "b3c"):
        bad[f"null {k}"] = dict(W_=dict(W, **{k: None}))
    for k in ("w2a", "b2a", "w3a", "b3a", "sigma"):
        bad[f"null {k} with logp_out"] = dict(W_=dict(W, **{k: None}))
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert "tsrl_ppo_eval" in _last_error() and "fused" not in _last_error(), \
            (what, _last_error())
        _untouched((v, n), (lp, n))
    assert call(n_=0) == 0
    _untouched((v, n), (lp, n))
    assert call() == 0   # the same buffers with good arguments
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v[:n]).all() and torch.isfinite(lp[:n]).all())


def test_fused_eval_refusals(dev):
    """tsrl_ppo_eval_fused returns non-zero, names itself in tsrl_last_error and leaves the
    NaN-filled outputs and workspace alone for: act_dim 0 and 33, logp_out without act, X,
    wsplit or the workspace 4 bytes off 16-byte alignment, ldx % 4 != 0, ldx < roundup(D, 4),
    ws_bytes one short, a NULL critic weight, a NULL actor weight with logp_out; n = 0 returns
    0 and writes nothing.  Every one of these returns before a launch."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    n, D, A = 33, 17, 6
    g = torch.Generator().manual_seed(4)
    W1 = {k: v.to(dev) for k, v in _l1_weights(g, D).items()}
    W = {k: v.to(dev) for k, v in _tail_weights(g, A).items()}
    X = torch.zeros(n, 24, device=dev)       # pitches 20 (good), 24; 16 and 18 are refused
    X[:, :D] = torch.randn(n, D, generator=g).to(dev)
    act = torch.randn(n, A, generator=g).to(dev)
    wsplit = _split_w(W1, D)
    nb = _fused_ws_bytes()
    evw = _out(nb // 4, dev)
    v, lp = _out(n, dev), _out(n, dev)

    def off4(t):
        o = torch.zeros(t.numel() + 4, device=dev)[1:]
        assert o.data_ptr() % 16 == 4
        return o

    def call(X_=X, ldx=24, n_=n, ws_=wsplit, W_=W, A_=A, act_=act, lp_=lp, evw_=evw, nb_=nb,
             actor=True):
        tw = _tw(W_, actor)
        return L.tsrl_ppo_eval_fused(_C.ptr(X_), ldx, None, n_, D, _C.ptr(ws_), _C.ptr(W1["b1a"]),
                                     _C.ptr(W1["b1c"]), tw, A_, _C.ptr(act_), _C.ptr(v),
                                     _C.ptr(lp_), _C.ptr(evw_), nb_, s)

    bad = {"act_dim 0": dict(A_=0), "act_dim 33": dict(A_=33),
           "logp_out without act": dict(act_=None),
           "X off alignment": dict(X_=off4(X)), "wsplit off alignment": dict(ws_=off4(wsplit)),
           "workspace off alignment": dict(evw_=off4(evw)),
           "ldx % 4": dict(ldx=18), "ldx < roundup(D, 4)": dict(ldx=16),
           "ws_bytes one short": dict(nb_=nb - 1),
           "null actor weights with logp_out": dict(actor=False)}
    for k in ("w2c", "b2c", "w3c", "b3c"):
        bad[f"null {k}"] = dict(W_=dict(W, **{k: None}))
    for k in ("w2a", "b2a", "w3a", "b3a", "sigma"):
        bad[f"null {k} with logp_out"] = dict(W_=dict(W, **{k: None}))
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert "tsrl_ppo_eval_fused" in _last_error(), (what, _last_error())
        _untouched((v, n), (lp, n), (evw, nb // 4))
    assert call(n_=0) == 0
    _untouched((v, n), (lp, n), (evw, nb // 4))
    for ldx in (20, 24):   # the same buffers with good arguments
        assert call(ldx=ldx) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(v[:n]).all() and torch.isfinite(lp[:n]).all())
    assert _canary_ok(v, n) and _canary_ok(lp, n) and _canary_ok(evw, nb // 4)


# =============================================================================================
# 5. Host paths around the kernels
# =============================================================================================
@pytest.mark.parametrize("use_idx", [False, True])
@pytest.mark.parametrize("with_act", [False, True])
def test_evaluate_chunk_loop_bitwise(dev, monkeypatch, use_idx, with_act):
    """5a: FusedActorCritic.evaluate in three chunks of 100, 100 and 57 rows (EVAL_CHUNK = 100,
    the two-kernel form: the pointer offsets of obs or idx, of act and of both outputs per
    chunk) has the bits of one chunk and of the fused form; table rows idx does not name are
    NaN."""
    import tianshou_amd.policy.fused_mlp as fm
    D, A, n = 8, 6, 257
    mlp = _policy(dev, D, A, 33)._mlp
    g = torch.Generator().manual_seed(5)
    N = n + 29 if use_idx else n
    obs = torch.randn(N, D, generator=g)
    idx = torch.randperm(N, generator=g)[:n] if use_idx else None
    if use_idx:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        obs[dead] = NAN
    obs = obs.to(dev)
    idx = None if idx is None else idx.to(dev)
    act = torch.randn(n, A, generator=g).to(dev) if with_act else None
    assert fm.FusedActorCritic.EVAL_CHUNK >= n
    monkeypatch.setattr(fm, "EVAL_FUSED", True)
    fused = mlp.evaluate(obs, act, idx)
    monkeypatch.setattr(fm, "EVAL_FUSED", False)
    one = mlp.evaluate(obs, act, idx)
    monkeypatch.setattr(fm.FusedActorCritic, "EVAL_CHUNK", 100)
    three = mlp.evaluate(obs, act, idx)
    torch.cuda.synchronize()
    for other in (one, fused):
        assert three[0].shape == (n,) and bool(torch.isfinite(three[0]).all())
        assert torch.equal(_bits(three[0]), _bits(other[0]))
        if with_act:
            assert bool(torch.isfinite(three[1]).all())
            assert torch.equal(_bits(three[1]), _bits(other[1]))
        else:
            assert three[1] is None and other[1] is None


def test_eval_values_shortcut_bitwise(dev):
    """5b: on a collected buffer (8 envs x 24 steps, episodes of 7 steps, so episode ends fall
    inside the per-env rows and every row ends mid-episode) FusedEvalMixin._eval_values takes
    V(s') from V(s) of the next row and evaluates obs_next only on the episode-end and
    segment-end rows: v_s_ and v_s have the bits of evaluate(obs_next) and evaluate(obs) over all rows; with
    buffer.obs_chain False it takes the full evaluation, with the same bits again."""
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    E, T, D, A = 8, 24, 8, 3
    pol = _policy(dev, D, A, 35)
    env = SyntheticVectorEnv(E, (D,), A, ep_len=7, seed=2, device=dev)
    buf = VectorReplayBuffer(E * T, E, device=dev)
    torch.manual_seed(4)
    Collector(pol, env, buf).collect(n_step=E * T)
    assert buf.obs_chain
    batch, idx = buf.sample(0)
    n = E * T
    assert len(idx) == n
    done = torch.as_tensor(batch.done).bool().reshape(n).cpu()
    ends = done.view(E, T)
    assert bool(ends[:, :-1].any()) and not bool(ends[:, :-1].all())
    mlp = pol._mlp
    calls = []
    orig = mlp.evaluate

    def spy(obs, act=None, idx=None):
        calls.append(None if idx is None else int(idx.numel()))
        return orig(obs, act, idx)

    with torch.no_grad():
        obs, obs_next = torch.as_tensor(batch.obs), torch.as_tensor(batch.obs_next)
        full_s, full_n = orig(obs)[0].clone(), orig(obs_next)[0].clone()
        mlp.evaluate = spy
        try:
            v_s, v_n = pol._eval_values(batch, obs, obs_next, buf, idx)
            short = list(calls)
            del calls[:]
            buf.obs_chain = False
            w_s, w_n = pol._eval_values(batch, obs, obs_next, buf, idx)
            long = list(calls)
        finally:
            mlp.evaluate = orig
            buf.obs_chain = True
    torch.cuda.synchronize()
    nend = int((done.view(E, T)[:, :-1]).sum()) + E
    assert short == [None, nend], short      # obs_next evaluated on the end rows only
    assert long == [None, None], long
    assert bool(torch.isfinite(full_s).all() and torch.isfinite(full_n).all())
    for a, b in ((v_s, full_s), (v_n, full_n), (w_s, full_s), (w_n, full_n)):
        assert torch.equal(_bits(a.contiguous()), _bits(b))
