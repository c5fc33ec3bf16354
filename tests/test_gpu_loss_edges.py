"""The PPO / A2C loss kernels (csrc/ppo.hip, csrc/ppo_cat.hip, csrc/ppo_loss.h) through the C
ABI, against the f64 references of tests/loss_edges_common.py, where the other loss tests'
inputs never go: -inf (masked) and extreme logits, probabilities that do not sum to 1, every
width around the 64 KiB LDS mark up to the limit of 64 and the argument error above it,
invalid action indices, Gaussian edge inputs, b_global != b, the advantage-moment kernels on
their own, and directed rows of the Gumbel-max sampler.

Tolerance (tests/test_gpu_noisy.py's rule): per output, err = the kernel's error against f64
and terr = the torch-f32 formulation's (run on the device, as there), both scaled by max |ref|;
floor = the largest terr over the case list (tests/loss_edges_common.py ``floors``; the two
cases whose f32 error is large by construction do not raise it); err <= max(4 * terr, floor).
Every case
prints err, terr and floor.  Rows whose branches f32 and f64 decide differently are compared
with the torch-f32 formulation alone (rtol 1e-4, atol 1e-6 * max |grad|).  Assertions that are
bit-exact or exactly zero say so.
"""
import numpy as np
import pytest
import torch

from . import loss_edges_common as lc

pytestmark = pytest.mark.gpu

SENT = -777.0  # prefilled into outputs a refused call must not write


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def refs(dev):
    """refs(name) -> (f64 reference, torch-f32 formulation, ambiguous rows) of a case, the
    torch-f32 formulation evaluated on the device as test_gpu_noisy.py's is (torch's f32
    arithmetic with the device's own exp and log); rows that this evaluation or the CPU's
    (tests/test_loss_edges_host.py) branches differently from f64 are ambiguous."""
    cache = {}

    def get(name):
        if name not in cache:
            r64, _, amb = lc.refs(name)
            r32 = lc.loss_ref(lc.CASES[name], torch.float32, dev)
            cache[name] = (r64, r32, amb | lc.ambiguous(r64, r32))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def floor(refs):
    return lc.floors(lc.CASES, refs)


def _params(p):
    from tianshou_amd import _C
    q = _C.PPOParams()
    q.objective = _C.OBJ_A2C if p["objective"] == "a2c" else _C.OBJ_PPO
    q.eps_clip, q.dual_clip = p["eps_clip"], p["dual_clip"]
    q.vf_coef, q.ent_coef, q.adv_eps, q.b_global = p["vf_coef"], p["ent_coef"], 1e-8, \
        float(p["b_global"])
    q.value_clip, q.norm_adv = int(p["value_clip"]), int(p["norm_adv"])
    return q


def _adv_sums(dev, case, adv):
    """(sum, sum of squares) of the minibatch advantages from the moment kernels, or of the
    global population in f64 when the case has one."""
    from tianshou_amd import _C
    if not case["p"]["norm_adv"]:
        return None
    if "adv_pop" in case:
        a = case["adv_pop"].double()
        return torch.stack([a.sum(), (a * a).sum()]).to(dev)
    L, s = _C.lib(), _C.stream_ptr(dev)
    B = case["B"]
    nblk = int(L.tsrl_ppo_num_partials(B))
    pa = torch.empty(nblk * 2, dtype=torch.float64, device=dev)
    _C.check(L.tsrl_adv_moments(_C.ptr(adv), None, B, _C.ptr(pa), s), "tsrl_adv_moments")
    out = torch.empty(2, dtype=torch.float64, device=dev)
    _C.check(L.tsrl_reduce_partials(_C.ptr(pa), nblk, 2, _C.ptr(out), s), "tsrl_reduce_partials")
    return out


def run_case(dev, case):
    """One launch of the case's loss kernel, reduction, finalize and log-prob kernel: the
    outputs of lc.outputs(kind) as CPU tensors."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    B, A, p = case["B"], case["A"], case["p"]
    ppo = p["objective"] == "ppo"
    value, adv, ret = d(case["value"]), d(case["adv"]), d(case["ret"])
    logp_old = d(case["logp_old"]) if ppo else None
    v_s = d(case["v_s"]) if p["value_clip"] else None
    adv_sums = _adv_sums(dev, case, adv)
    nblk = int(L.tsrl_ppo_num_partials(B))
    grad_value = torch.full((B,), SENT, device=dev)
    terms = torch.full((4,), SENT, device=dev)
    logp = torch.full((B,), SENT, device=dev)
    out = {}
    if case["kind"] == "cat":
        x, act = d(case["x"]), d(case["act"])
        grad_x = torch.full((B, A), SENT, device=dev)
        partials = torch.empty(nblk * 4, dtype=torch.float64, device=dev)
        _C.check(L.tsrl_ppo_cat_fwd_bwd(
            _C.ptr(x), _C.ptr(value), _C.ptr(act), _C.ptr(logp_old), _C.ptr(adv), _C.ptr(ret),
            _C.ptr(v_s), None, B, A, case["mode"], _C.ptr(adv_sums), _params(p), _C.ptr(grad_x),
            _C.ptr(grad_value), _C.ptr(partials), s), "tsrl_ppo_cat_fwd_bwd")
        sums = torch.empty(4, dtype=torch.float64, device=dev)
        _C.check(L.tsrl_reduce_partials(_C.ptr(partials), nblk, 4, _C.ptr(sums), s), "reduce")
        _C.check(L.tsrl_ppo_cat_finalize(_C.ptr(sums), _params(p), _C.ptr(terms), s), "finalize")
        _C.check(L.tsrl_cat_logp(_C.ptr(x), _C.ptr(act), B, A, case["mode"], _C.ptr(logp), s),
                 "tsrl_cat_logp")
        out["grad_x"] = grad_x
    else:
        mu, ls, act = d(case["mu"]), d(case["log_std"]), d(case["act"])
        grad_mu = torch.full((B, A), SENT, device=dev)
        grad_ls = torch.full((A,), SENT, device=dev)
        partials = torch.empty(nblk * (4 + A), dtype=torch.float64, device=dev)
        _C.check(L.tsrl_ppo_gauss_fwd_bwd(
            _C.ptr(mu), _C.ptr(ls), _C.ptr(value), _C.ptr(act), _C.ptr(logp_old), _C.ptr(adv),
            _C.ptr(ret), _C.ptr(v_s), None, B, A, _C.ptr(adv_sums), _params(p), _C.ptr(grad_mu),
            _C.ptr(grad_value), _C.ptr(partials), s), "tsrl_ppo_gauss_fwd_bwd")
        sums = torch.empty(4 + A, dtype=torch.float64, device=dev)
        _C.check(L.tsrl_reduce_partials(_C.ptr(partials), nblk, 4 + A, _C.ptr(sums), s),
                 "reduce")
        _C.check(L.tsrl_ppo_gauss_finalize(_C.ptr(sums), A, _C.ptr(ls), _params(p),
                                           _C.ptr(terms), _C.ptr(grad_ls), s), "finalize")
        _C.check(L.tsrl_gauss_logp(_C.ptr(mu), _C.ptr(ls), _C.ptr(act), B, A, _C.ptr(logp), s),
                 "tsrl_gauss_logp")
        out["grad_mu"], out["grad_ls"] = grad_mu, grad_ls
    out.update(grad_value=grad_value, logp=logp)
    out = {k: v.cpu() for k, v in out.items()}
    out.update(zip(lc.TERMS, terms.cpu()))
    return out


def check_case(name, got, floor, refs):
    case = lc.CASES[name]
    r64, r32, amb = refs(name)
    assert float(amb.double().mean()) <= 0.01
    bad = []
    for o in lc.outputs(case["kind"]):
        keep = ~amb if o in lc.ROW_GRADS else None
        err = lc.scaled_err(got[o], r64[o], keep)
        terr = lc.scaled_err(r32[o], r64[o], keep)
        fl = floor.get((case["kind"], o), 0.0)
        print(f"{name} {o}: err {err:.2e} terr {terr:.2e} floor {fl:.2e}"
              f" ({int(amb.sum())} ambiguous rows)")
        if not err <= max(4 * terr, fl):
            bad.append((o, err, terr, fl))
        if o in lc.ROW_GRADS:
            lc.check_ambiguous_rows(got[o], r32, amb, o)
    assert not bad, bad


# -- 1: masked logits ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.names("masked"))
def test_masked_logits(dev, floor, refs, name):
    """-inf logits, PPO and A2C objectives: terms, gradients and tsrl_cat_logp against f64;
    the gradient is exactly 0 at every masked entry and finite everywhere."""
    case = lc.CASES[name]
    got = run_case(dev, case)
    masked = case["x"] == -lc.INF
    g = got["grad_x"]
    print(f"{name}: {int(torch.isnan(g).sum())} NaN of {g.numel()} gradient entries, "
          f"{int(masked.sum())} masked")
    assert bool(torch.isfinite(g).all()), "non-finite grad_x"
    assert bool((g[masked] == 0).all()), "exactly 0 at masked entries"
    assert all(bool(torch.isfinite(got[o])) for o in lc.TERMS)
    check_case(name, got, floor, refs)


# -- 2: extreme finite logits ----------------------------------------------------------------------
def test_extreme_logits(dev, floor, refs):
    got = run_case(dev, lc.CASES["extreme"])
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    check_case("extreme", got, floor, refs)


def test_one_action(dev, floor, refs):
    """A = 1: log-prob, entropy and gradient are exactly 0."""
    got = run_case(dev, lc.CASES["one-action"])
    assert not got["logp"].any() and not got["grad_x"].any() and float(got["ent"]) == 0.0
    check_case("one-action", got, floor, refs)


# -- 3: unnormalised probabilities -------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.names("probs"))
def test_unnormalised_probs(dev, floor, refs, name):
    """Categorical(probs=x) with row sums of 0.25, 1, 3 and 1e-3.  A row times 3 has a third
    of the gradient: 3 * grad of rows [PAIRS, 2 PAIRS) against the f64 gradient of rows
    [0, PAIRS), under the same rule (a missing / S fails it by a factor of 3)."""
    got = run_case(dev, lc.CASES[name])
    check_case(name, got, floor, refs)
    r64, r32, amb = refs(name)
    P = lc.PAIRS
    keep = ~(amb[:P] | amb[P:2 * P])
    want = r64["grad_x"][:P]
    err = lc.scaled_err(3 * got["grad_x"][P:2 * P], want, keep)
    terr = lc.scaled_err(3 * r32["grad_x"][P:2 * P], want, keep)
    fl = floor[("cat", "grad_x")]
    print(f"{name} 3 * grad_x[c=3] vs grad_x[c=1]: err {err:.2e} terr {terr:.2e} floor {fl:.2e}")
    assert float(want.abs().max()) > 0 and err <= max(4 * terr, fl)


# -- 4: width limits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.names("width"))
def test_widths(dev, floor, refs, name):
    got = run_case(dev, lc.CASES[name])
    check_case(name, got, floor, refs)


def test_width_65_is_refused(dev):
    """65 actions: every entry point returns nonzero and writes none of its outputs."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    B, A = 257, 65
    z = lambda *sh: torch.zeros(*sh, device=dev)  # noqa: E731
    full = lambda *sh: torch.full(sh, SENT, device=dev)  # noqa: E731
    act_i = torch.zeros(B, dtype=torch.int64, device=dev)
    p = _params(dict(lc.PPO, b_global=B))
    nblk = int(L.tsrl_ppo_num_partials(B))
    gx, gv, lp, terms, gls = full(B, A), full(B), full(B), full(4), full(A)
    part = torch.full((nblk * (4 + A),), SENT, dtype=torch.float64, device=dev)
    sums = torch.zeros(4 + A, dtype=torch.float64, device=dev)
    rcs = dict(
        gauss_fwd_bwd=L.tsrl_ppo_gauss_fwd_bwd(
            _C.ptr(z(B, A)), _C.ptr(z(A)), _C.ptr(z(B)), _C.ptr(z(B, A)), _C.ptr(z(B)),
            _C.ptr(z(B)), _C.ptr(z(B)), None, None, B, A, None, p, _C.ptr(gx), _C.ptr(gv),
            _C.ptr(part), s),
        cat_fwd_bwd=L.tsrl_ppo_cat_fwd_bwd(
            _C.ptr(z(B, A)), _C.ptr(z(B)), _C.ptr(act_i), _C.ptr(z(B)), _C.ptr(z(B)),
            _C.ptr(z(B)), None, None, B, A, 0, None, p, _C.ptr(gx), _C.ptr(gv), _C.ptr(part),
            s),
        gauss_logp=L.tsrl_gauss_logp(_C.ptr(z(B, A)), _C.ptr(z(A)), _C.ptr(z(B, A)), B, A,
                                     _C.ptr(lp), s),
        cat_logp=L.tsrl_cat_logp(_C.ptr(z(B, A)), _C.ptr(act_i), B, A, 0, _C.ptr(lp), s),
        gauss_finalize=L.tsrl_ppo_gauss_finalize(_C.ptr(sums), A, _C.ptr(z(A)), p,
                                                 _C.ptr(terms), _C.ptr(gls), s))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in rcs.values()), rcs
    for t in (gx, gv, lp, terms, gls, part):
        assert bool((t == SENT).all())  # exactly the sentinel: nothing was written


# -- 5: invalid action index ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_invalid_action_index(dev, mode):
    """act of -1 and of A in two rows: their log-prob is NaN, and every other row's gradients
    are bit for bit those of the launch with valid actions in the two rows (rows are
    independent, and the guard keeps the read inside the row)."""
    B, A = 257, 6
    case, g = lc._base(50 + mode, "cat", B, A, mode, norm_adv=True, value_clip=True)
    lc._finish(case, g)
    bad = dict(case, act=case["act"].clone())
    bad["act"][3], bad["act"][B - 1] = -1, A
    got, want = run_case(dev, bad), run_case(dev, case)
    rows = torch.ones(B, dtype=torch.bool)
    rows[3] = rows[B - 1] = False
    assert bool(torch.isnan(got["logp"][~rows]).all())
    assert torch.equal(got["logp"][rows], want["logp"][rows])           # bit-exact
    assert torch.equal(got["grad_x"][rows], want["grad_x"][rows])       # bit-exact
    assert torch.equal(got["grad_value"], want["grad_value"])           # bit-exact, all rows
    assert bool(torch.isfinite(want["grad_x"]).all())


# -- 6: Gaussian inputs ---------------------------------------------------------------------------------
def test_gauss_edges(dev, floor, refs):
    """log_std of -5, 0 and 2 in one case, rows 8 sigma out, and rows with act == mu, whose
    d/d mu is exactly 0."""
    case = lc.CASES["gauss-edge"]
    got = run_case(dev, case)
    assert not got["grad_mu"][:case["exact_rows"]].any()  # exactly 0
    assert bool(got["grad_mu"][case["exact_rows"]:].any())
    check_case("gauss-edge", got, floor, refs)


# -- 7: b_global != b -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.names("global"))
def test_global_minibatch(dev, floor, refs, name):
    """257 local rows of a 771-row global minibatch: gradients scaled by 1 / 771, terms = local
    sums / 771, advantages normalised by the population's moments (given as f64 sums)."""
    assert lc.CASES[name]["p"]["b_global"] == 3 * lc.CASES[name]["B"]
    check_case(name, run_case(dev, lc.CASES[name]), floor, refs)


# -- 8: advantage moments ---------------------------------------------------------------------------------
def _sums64(a):
    a = a.double().numpy()
    return np.array([a.sum(), (a * a).sum()])


def _check_sums(got, vals, what):
    """f64 sums of n f32 values (all of one sign, no cancellation): n * 2^-52 relative."""
    want = _sums64(vals)
    n = max(len(vals), 1)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{what}: n {len(vals)} rel err {err.max():.2e} (allowed {n * 2.0 ** -52:.2e})")
    assert (err <= n * 2.0 ** -52).all() if len(vals) else not got.any()


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("b", [1, 255, 256, 257, 4097])
def test_adv_moments(dev, b, gather):
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    g = torch.Generator().manual_seed(b + gather)
    n = b + 100 if gather else b
    adv = torch.randn(n, generator=g) + 1e4
    idx = torch.randperm(n, generator=g)[:b] if gather else None
    nblk = int(L.tsrl_ppo_num_partials(b))
    assert nblk == (b + 255) // 256
    pa = torch.empty(nblk * 2, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    adv_d = adv.to(dev)
    idx_d = idx.to(dev) if gather else None
    _C.check(L.tsrl_adv_moments(_C.ptr(adv_d), _C.ptr(idx_d), b, _C.ptr(pa), s), "moments")
    _C.check(L.tsrl_reduce_partials(_C.ptr(pa), nblk, 2, _C.ptr(out), s), "reduce")
    _check_sums(out.cpu().numpy(), adv[idx] if gather else adv, f"adv_moments b={b}")


def _run_seg(dev, adv, idx, bounds):
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    nseg = len(bounds) - 1
    max_seg = max(bounds[i + 1] - bounds[i] for i in range(nseg))
    nparts = int(L.tsrl_adv_moments_seg_parts(max_seg))
    partials = torch.empty(nseg * nparts * 2, dtype=torch.float64, device=dev)
    out = torch.full((nseg * 2,), SENT, dtype=torch.float64, device=dev)
    adv_d, b_d = adv.to(dev), torch.tensor(bounds, dtype=torch.int64, device=dev)
    idx_d = None if idx is None else idx.to(dev)
    _C.check(L.tsrl_adv_moments_seg(_C.ptr(adv_d), _C.ptr(idx_d), _C.ptr(b_d), nseg, max_seg,
                                    _C.ptr(partials), _C.ptr(out), s), "tsrl_adv_moments_seg")
    return out.cpu().numpy().reshape(nseg, 2), nparts


@pytest.mark.parametrize("gather", [False, True])
def test_adv_moments_seg(dev, gather):
    """An empty segment (sums exactly 0), a one-row segment and unequal ones."""
    g = torch.Generator().manual_seed(80 + gather)
    bounds = [0, 0, 1, 256, 1000, 4097]
    adv = torch.randn(4097, generator=g) + 1e4
    idx = torch.randperm(4097, generator=g) if gather else None
    got, nparts = _run_seg(dev, adv, idx, bounds)
    assert nparts == 4
    src = adv[idx] if gather else adv
    for k in range(len(bounds) - 1):
        _check_sums(got[k], src[bounds[k]:bounds[k + 1]], f"segment {k}")
    assert not got[0].any()  # exactly 0


def test_adv_moments_seg_parts_clamp(dev):
    """max_seg = 4 * 256 * 256 + 1 asks for 257 parts and gets the clamp of 256: each
    workgroup then strides over its share more than once."""
    from tianshou_amd import _C
    n0 = 4 * 256 * 256 + 1
    assert int(_C.lib().tsrl_adv_moments_seg_parts(n0)) == 256
    assert int(_C.lib().tsrl_adv_moments_seg_parts(n0 - 1)) == 256
    assert int(_C.lib().tsrl_adv_moments_seg_parts(1)) == 1
    g = torch.Generator().manual_seed(81)
    bounds = [0, n0, n0 + 1000]
    adv = torch.randn(bounds[-1], generator=g) + 1e4
    got, nparts = _run_seg(dev, adv, None, bounds)
    assert nparts == 256
    for k in range(2):
        _check_sums(got[k], adv[bounds[k]:bounds[k + 1]], f"clamped segment {k}")


@pytest.mark.parametrize("width", [2, 4 + 64])
@pytest.mark.parametrize("nblk", [1, 255, 257])
def test_reduce_partials(dev, nblk, width):
    from tianshou_amd import _C
    g = torch.Generator().manual_seed(nblk + width)
    part = torch.rand(nblk, width, generator=g, dtype=torch.float64) + 0.5
    out = torch.empty(width, dtype=torch.float64, device=dev)
    part_d = part.to(dev)
    _C.check(_C.lib().tsrl_reduce_partials(_C.ptr(part_d), nblk, width, _C.ptr(out),
                                           _C.stream_ptr(dev)), "tsrl_reduce_partials")
    want = part.numpy().sum(0)
    err = np.abs(out.cpu().numpy() - want) / want
    print(f"reduce_partials nblk={nblk} width={width}: rel err {err.max():.2e}")
    assert (err <= nblk * 2.0 ** -52).all()


def test_shifted_advantages_through_loss(dev, floor, refs):
    """Advantages of mean 1e4 and std 1 through a loss launch with norm_adv: the kernel's
    mean and std (adv_mean_std, from f64 sums) against the f64 moments."""
    check_case("shifted-adv", run_case(dev, lc.CASES["shifted-adv"]), floor, refs)


# -- 9: Gumbel-max sampler, directed rows -------------------------------------------------------------------
def _gumbel(dev, logits, u):
    from tianshou_amd import _C
    n, A = logits.shape
    out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    lg, ud = logits.to(dev).contiguous(), u.to(dev).contiguous()
    _C.check(_C.lib().tsrl_cat_gumbel_argmax(_C.ptr(lg), _C.ptr(ud), n, A, _C.ptr(out),
                                             _C.stream_ptr(dev)), "tsrl_cat_gumbel_argmax")
    return out.cpu()


@pytest.mark.parametrize("A", [2, 6, 18])
def test_gumbel_never_draws_masked(dev, A):
    n = 4096
    g = torch.Generator().manual_seed(90 + A)
    logits = torch.randn(n, A, generator=g) * 1.5
    k = 1 + torch.arange(n) % (A - 1)  # masked entries per row
    order = torch.argsort(torch.rand(n, A, generator=g), dim=1)
    masked = torch.zeros(n, A, dtype=torch.bool)
    masked.scatter_(1, order, torch.arange(A).expand(n, A) < k.unsqueeze(1))
    logits[masked] = -lc.INF
    u = torch.rand(n, A, generator=g)
    assert bool((u > 0).all()) and bool((~masked).any(1).all())
    a = _gumbel(dev, logits, u)
    assert bool((a >= 0).all()) and bool((a < A).all())
    assert not bool(masked[torch.arange(n), a].any())
    # rows with one finite logit always return it (k == A - 1)
    one = k == A - 1
    assert bool(one.any())
    assert torch.equal(a[one], (~masked[one]).float().argmax(1))


def test_gumbel_directed_rows(dev):
    A = 6
    g = torch.Generator().manual_seed(99)
    # u = 0 at an entry (Gumbel noise -inf) never selects it while another entry is finite,
    # however large its logit
    logits = torch.randn(A, A, generator=g)
    u = torch.rand(A, A, generator=g).clamp_(min=1e-3)
    for i in range(A):
        u[i, i] = 0.0
        logits[i, i] = 50.0
    a = _gumbel(dev, logits, u)
    assert not bool((a == torch.arange(A)).any())
    # equal logits with equal u: the first index
    a = _gumbel(dev, torch.full((4, A), 0.7), torch.full((4, A), 0.3))
    assert not a.any()
