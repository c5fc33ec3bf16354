"""References and case builders shared by tests/test_optim_edges_host.py (CPU) and
tests/test_gpu_optim_edges.py (GPU): tsrl_clip_adam / tsrl_clip_rmsprop of csrc/optim.hip at
eps, step-count, slice, clip and overflow edges.  NumPy, torch on the CPU and the standard
library only; nothing here touches a device.

``step_ref`` is the f64 statement of one launch (clip_grad_norm_ + Adam / RMSprop) on the
hyperparameters as the C ABI's ``float`` arguments carry them; ``step_f32`` is the same formula
one f32 torch op at a time in the kernel's order of operations, whose own error against
``step_ref`` (``terr``) scales the bound on the kernel's update.

Bounds, all derived (u = 2^-24, the f32 unit roundoff; eta = 2^-149, the f32 denormal spacing,
the absolute error one operation can add under gradual underflow):

* ``m``: |got - ref| <= K_M u (|b1 m| + |(1-b1) gi|) + K_M eta.  f32 roundings on the path:
  gi = g coef (1), 1 - b1 (1; exact for b1 >= 0.5), b1 m (1), (1-b1) gi (1), the sum (1) = 5,
  + 1 for a fused multiply-add that rounds differently = K_M 6.  With clipping the kernel's
  coefficient may sit 2 ulp from the reference's (the bound on norm_out[1]): + 2 = 8.
* ``v``: |got - ref| <= K_V u (|b2 v| + |(1-b2) gi^2|) + K_V eta.  gi enters twice (2), 1 - b2
  (1), b2 v (1), (1-b2) gi (1), that times gi (1), the sum (1) = 7, + 1 FMA = K_V 8; with
  clipping the coefficient's 2 ulp enter twice: + 4 = 12.  An entry whose reference is below
  f32's smallest normal (2^-126) may also be exactly 0.
* the update (parameters started at 0.0, so p_new = -update at full f32 precision):
  elementwise relative error err <= max(4 terr, floor), floor the largest terr over the cases
  that count (every case of fixed size but the overflow one).
* parameters started at N(0,1): |got - ref| <= ulp32(ref) + max(4 terr, floor) |update|.
* norm_out[0] within 1 f32 ulp of the correctly rounded exact norm (the kernel's f64 sum over
  n <= 6e5 terms is off by at most n 2^-53 ~ 7e-11 relative, far below half an f32 ulp);
  norm_out[1] within 2 ulp of the reference coefficient (the norm's 1 ulp through the add and
  the divide), and exactly 1.0 where the reference clamps.
"""
import functools
import math

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
ETA = 2.0 ** -149
TINY = 2.0 ** -126  # f32's smallest normal
OCHUNK = 2048  # elements per workgroup of clip_step_kernel
SCALE_SPAN = 1024 * 256  # elements of one trip of clip_scale_kernel's grid
N0 = 4097

ADAM = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)
RMS = dict(lr=7e-4, alpha=0.99, eps=1e-5)
KINDS = ("adam", "rmsprop")


def defaults(kind, **kw):
    return dict(ADAM if kind == "adam" else RMS, **kw)


def as_f32(hyper):
    """The hyperparameters as the C ABI's float arguments carry them (Python floats)."""
    return {k: float(F32(x)) for k, x in hyper.items()}


# ---------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------
def exact_norm(g):
    """sqrt of the exactly summed squares (a f32 square is exact in f64; math.fsum rounds the
    sum once).  inf with an infinite element, NaN with a NaN one."""
    x = np.asarray(g, np.float64)
    if np.isnan(x).any():
        return math.nan
    return math.sqrt(math.fsum((x * x).tolist()))


def clip_ref(g, max_norm):
    """(norm32, coef32) of clip_grad_norm_: the exact norm rounded once to f32, the
    coefficient in f32 steps -- max_norm / (norm + 1e-6f), coef > 1 -> 1; NaN stays NaN."""
    with np.errstate(all="ignore"):
        norm = F32(exact_norm(g))
        coef = F32(max_norm) / (norm + F32(1e-6))
        if coef > F32(1.0):
            coef = F32(1.0)
    return norm, coef


def torch_f32_clip(g, max_norm):
    """(norm, non-zero gradients left) of torch.nn.utils.clip_grad_norm_ on the f32 gradient
    on the CPU; reported beside the kernel's where the two differ, never asserted."""
    t = torch.nn.Parameter(torch.zeros(len(g)))
    t.grad = torch.from_numpy(np.array(g, F32))
    norm = float(torch.nn.utils.clip_grad_norm_([t], max_norm))
    return norm, int(torch.count_nonzero(t.grad))


def step_ref(kind, p, g, m, v, t0, hyper, max_norm, double_hyper=False):
    """One launch in float64.  hyper / max_norm are rounded to f32 first (double_hyper: kept
    as Python doubles, torch's semantics; only the deviation is reported from it).  Returns a
    dict: p, m, v, update (= p_old - p_new before any rounding), gi (the clipped gradient),
    norm, coef (f32; None unclipped), and the terms of the m / v bounds."""
    h = dict(hyper) if double_hyper else as_f32(hyper)
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    v = np.asarray(v, np.float64)
    t = float(t0 + 1)
    norm = coef = None
    out = {}
    with np.errstate(all="ignore"):
        gi = g
        if max_norm:
            norm, coef = clip_ref(g, max_norm)
            gi = g * float(coef)
        if kind == "adam":
            m = np.asarray(m, np.float64)
            b1, b2 = h["beta1"], h["beta2"]
            ta, tb = b1 * m, (1.0 - b1) * gi
            m = ta + tb
            out["m_terms"] = np.abs(ta) + np.abs(tb)
            ta, tb = b2 * v, (1.0 - b2) * gi * gi
            v = ta + tb
            upd = h["lr"] / (1.0 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t)
                                                  + h["eps"])
        else:
            a = h["alpha"]
            ta, tb = a * v, (1.0 - a) * gi * gi
            v = ta + tb
            m = None
            upd = h["lr"] * gi / (np.sqrt(v) + h["eps"])
        out["v_terms"] = np.abs(ta) + np.abs(tb)
        out.update(p=p - upd, m=m, v=v, update=upd, gi=gi, norm=norm, coef=coef)
    return out


def step_f32(kind, p, g, m, v, t0, hyper, max_norm):
    """The same formula one f32 torch op at a time on the CPU, in the order of operations of
    AdamRule / RmspropRule (csrc/optim.hip): ((1-b2) gi) gi, (step_size m) / denominator.  The
    clip coefficient is the reference's (an f32 quantity by definition)."""
    T = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    A = lambda x: torch.from_numpy(np.array(x, np.float32))  # noqa: E731
    p, gi, v = A(p), A(g), A(v)
    if max_norm:
        gi = gi * T(float(clip_ref(g, max_norm)[1]))
    t, one = T(float(t0 + 1)), T(1.0)
    if kind == "adam":
        m = A(m)
        b1, b2 = T(hyper["beta1"]), T(hyper["beta2"])
        bc1 = one - torch.pow(b1, t)
        bc2_sqrt = torch.sqrt(one - torch.pow(b2, t))
        step_size = T(hyper["lr"]) / bc1
        m = b1 * m + (one - b1) * gi
        v = b2 * v + ((one - b2) * gi) * gi
        p = p - (step_size * m) / (torch.sqrt(v) / bc2_sqrt + T(hyper["eps"]))
    else:
        a = T(hyper["alpha"])
        v = a * v + ((one - a) * gi) * gi
        m = None
        p = p - (T(hyper["lr"]) * gi) / (torch.sqrt(v) + T(hyper["eps"]))
    assert p.dtype == v.dtype == torch.float32
    return dict(p=p.numpy(), m=None if m is None else m.numpy(), v=v.numpy())


# ---------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------
def make_case(name, kind, g, t0=9, max_norm=None, seed=0, zero_state=False, state=None,
              floor=True, **hyper):
    """g (cast to f32) with a state consistent with t0 earlier steps of gradients of the same
    sign and size as the clipped gradient gi: m = (1 - b1^t0) gi u, v = (1 - b2^t0) gi^2 w, u
    and w uniform in [0.5, 1.5) (zeros at t0 = 0).  Same signs, so neither moment cancels and
    the update's elementwise relative error measures the kernel, not the conditioning of
    b1 m + (1-b1) g (the m / v bounds, in terms of the summands, hold either way)."""
    h = defaults(kind, **hyper)
    g = np.ascontiguousarray(np.asarray(g, np.float64).astype(F32))
    n = len(g)
    rng = np.random.default_rng(1000 + seed)
    hf = as_f32(h)
    with np.errstate(all="ignore"):
        gi = g.astype(np.float64)
        if max_norm and np.isfinite(g).all():  # (an infinite element: the state of the raw g)
            gi = gi * float(clip_ref(g, max_norm)[1])
        gi = np.where(np.isfinite(gi), gi, 1.0)
        b2 = hf["beta2"] if kind == "adam" else hf["alpha"]
        u, w = rng.uniform(0.5, 1.5, n), rng.uniform(0.5, 1.5, n)
        if state is not None:
            m0, v0 = state
        elif zero_state or t0 == 0:
            m0, v0 = np.zeros(n), np.zeros(n)
        else:
            m0 = (1.0 - hf.get("beta1", 0.0) ** t0) * gi * u
            v0 = (1.0 - b2 ** t0) * gi * gi * w
        m0, v0 = np.asarray(m0, np.float64).astype(F32), np.asarray(v0, np.float64).astype(F32)
    assert t0 > 0 or (not m0.any() and not v0.any())
    return dict(name=f"{kind} {name}", kind=kind, hyper=h, g=g, m0=m0 if kind == "adam" else None,
                v0=v0, t0=t0, max_norm=max_norm, n=n, seed=seed, floor=floor)


def p_start(c, which):
    """The parameter vector a case starts from: "zero" or "randn"."""
    if which == "zero":
        return np.zeros(c["n"], F32)
    return np.random.default_rng(7000 + c["seed"]).standard_normal(c["n"]).astype(F32)


def _randn(seed, n=N0):
    return np.random.default_rng(seed).standard_normal(n)


T0S = (0, 1, 9, 999, 99999)
G_SCALES = (1e-4, 1.0, 1e4)


def cases_plain(kind):
    return [make_case(f"plain g={s:g} t0={t0}", kind, _randn(10 + i) * s, t0=t0, seed=10 + i)
            for i, (s, t0) in enumerate((s, t0) for s in G_SCALES for t0 in T0S)]


MIXED_SHARE = (0.6, 0.9)  # share of the mixed case's elements with sqrt(v_hat) < eps


def cases_eps(kind):
    """eps-dominated: sqrt(v_hat) < eps on every element; for Adam also the mixed regime of
    Rainbow-style settings (eps 1.5e-4, lr 6.25e-5, g ~ 1e-4 N(0,1)), where sqrt(v_hat) < eps
    on a share of the elements inside MIXED_SHARE; for RMSprop also FQF's fraction optimiser
    (lr 2.5e-9, eps 1e-5)."""
    out = [make_case(f"eps-dominated t0={t0}", kind, _randn(40 + t0) * 1e-10, t0=t0, seed=40,
                     eps=1e-8) for t0 in (0, 9)]
    if kind == "adam":
        out += [make_case(f"eps-mixed t0={t0}", kind, _randn(42 + t0) * 1e-4, t0=t0, seed=42,
                          eps=1.5e-4, lr=6.25e-5) for t0 in (0, 999)]
    else:
        out += [make_case(f"eps-dominated lr=2.5e-9 t0={t0}", kind, _randn(44 + t0) * 1e-10,
                          t0=t0, seed=44, eps=1e-5, lr=2.5e-9) for t0 in (0, 999)]
    return out


def sqrt_vhat(c):
    """sqrt of the bias-corrected second moment after the case's step (f64)."""
    r = step_ref(c["kind"], p_start(c, "zero"), c["g"], c["m0"], c["v0"], c["t0"], c["hyper"],
                 c["max_norm"])
    if c["kind"] == "rmsprop":
        return np.sqrt(r["v"])
    return np.sqrt(r["v"] / (1.0 - as_f32(c["hyper"])["beta2"] ** (c["t0"] + 1)))


def cases_zeros(kind):
    """g = 0 with non-zero moments (decay only), and with m = v = 0 (the update is exactly 0:
    0 / (0 + eps), never 0 / 0, because eps > 0)."""
    rng = np.random.default_rng(50)
    m0, v0 = rng.standard_normal(N0) * 0.1, rng.uniform(0.5, 1.5, N0) * 0.01
    return [make_case("zeros decay-only", kind, np.zeros(N0), t0=999, state=(m0, v0), seed=50),
            make_case("zeros all-zero t0=0", kind, np.zeros(N0), t0=0, seed=51),
            make_case("zeros all-zero t0=999", kind, np.zeros(N0), t0=999, zero_state=True,
                      seed=52)]


def cases_tiny(kind):
    return [make_case(f"tiny t0={t0}", kind, _randn(60 + t0) * 1e-20, t0=t0, seed=60)
            for t0 in (0, 9)]


def cases_huge(kind):
    """1e18 N(0,1) unclipped: every product of the kernel's formula is finite in f32.  1e25
    N(0,1) clipped at 0.5: the squares overflow f32, the f64 norm does not."""
    return [make_case("huge 1e18 unclipped", kind, _randn(70) * 1e18, t0=9, seed=70),
            make_case("huge 1e25 clipped", kind, _randn(71) * 1e25, t0=9, max_norm=0.5, seed=71)]


OVERFLOW_POS_1E20 = (3, 2047, 2048, 4096)
OVERFLOW_POS_1E21 = (5, 2049, 4095)


def case_overflow(kind):
    """N(0,1) with |g| = 1e20 at OVERFLOW_POS_1E20 and |g| = 1e21 at OVERFLOW_POS_1E21,
    unclipped, from the zero state.  g^2 alone overflows f32 at both, but the kernel never
    forms it: ((1-b2) g) g is 1e37 (Adam) / 1e38 (RMSprop) at 1e20, finite and held to the
    normal bounds, and inf at 1e21 (the threshold is sqrt(FLT_MAX / (1-b2)): 5.8e20 for Adam's
    0.999, 1.8e20 for RMSprop's 0.99), where f64's 1e39 is finite: there the expected values
    are step_f32's."""
    g = _randn(80)
    for k, i in enumerate(OVERFLOW_POS_1E20):
        g[i] = 1e20 * (-1) ** k
    for k, i in enumerate(OVERFLOW_POS_1E21):
        g[i] = 1e21 * (-1) ** k
    return make_case("overflow", kind, g, t0=0, seed=80, floor=False)


def overflow_second_gradient():
    """An ordinary N(0,1) gradient for the step after the overflow: v must stay at inf."""
    return _randn(81).astype(F32)


INF_POS = {"+inf": ((1000, np.inf),), "-inf": ((4096, -np.inf),),
           "both": ((2047, np.inf), (2048, -np.inf))}


def cases_inf(kind):
    out = []
    for name, places in INF_POS.items():
        for max_norm in (None, 0.5):
            g = _randn(90)
            for i, x in places:
                g[i] = x
            out.append(make_case(f"inf {name} max_norm={max_norm}", kind, g, t0=9,
                                 max_norm=max_norm, seed=90))
    return out


def scaled_to_norm(seed, target, n=N0):
    """N(0,1) scaled (in f64, then cast) so that its exact norm is target to ~1e-9 relative."""
    g = _randn(seed, n)
    return (g * (target / exact_norm(g))).astype(F32)


# (name, max_norm, exact norm, whether the coefficient clamps to 1).  The clamp is at
# norm + 1e-6 = max_norm, so max_norm (1 +- 2^-20) straddles it only where max_norm 2^-20 >
# 1e-6: at 4.0 it does; at 0.5 both sides scale (coefficients 0.999997 and 0.999999), and the
# pair around 0.5 - 1e-6 is the one that straddles.
NORM_EDGES = (
    ("norm=4(1-2^-20)", 4.0, 4.0 * (1 - 2.0 ** -20), True),
    ("norm=4(1+2^-20)", 4.0, 4.0 * (1 + 2.0 ** -20), False),
    ("norm=.5(1-2^-20)", 0.5, 0.5 * (1 - 2.0 ** -20), False),
    ("norm=.5(1+2^-20)", 0.5, 0.5 * (1 + 2.0 ** -20), False),
    ("norm=(.5-1e-6)(1-2^-20)", 0.5, (0.5 - 1e-6) * (1 - 2.0 ** -20), True),
    ("norm=(.5-1e-6)(1+2^-20)", 0.5, (0.5 - 1e-6) * (1 + 2.0 ** -20), False),
)


def cases_norm_edges(kind):
    out = [make_case("norm all-zero clipped", kind, np.zeros(N0), t0=0, max_norm=0.5, seed=100)]
    for i, (name, max_norm, target, _) in enumerate(NORM_EDGES):
        out.append(make_case(name, kind, scaled_to_norm(101 + i, target), t0=9,
                             max_norm=max_norm, seed=101 + i))
    out += [make_case(f"max_norm={mn:g}", kind, _randn(110), t0=9, max_norm=mn, seed=110)
            for mn in (1e-30, 1e30)]
    return out


def regime_cases(kind):
    """Every fixed-size case but the overflow one and the sizes."""
    return (cases_plain(kind) + cases_eps(kind) + cases_zeros(kind) + cases_tiny(kind)
            + cases_huge(kind) + cases_inf(kind) + cases_norm_edges(kind))


SIZES = (1, 255, 256, 257, 2047, 2048, 2049, 4097, SCALE_SPAN - 1, SCALE_SPAN, SCALE_SPAN + 1)
MARKER = dict(g=3.0, m=0.25, v=4.0, p=1.5)


def case_size(kind, n, max_norm):
    """g ~ N(0,1), t0 = 9, with a marker in the last element: g 3.0, m 0.25, v 4.0 (p 1.5 in
    the randn start), in range and finite, its update whatever step_ref says."""
    c = make_case(f"size n={n} max_norm={max_norm}", kind, _randn(120 + n % 1000, n), t0=9,
                  max_norm=max_norm, seed=120)
    c["g"][-1] = MARKER["g"]
    c["v0"][-1] = MARKER["v"]
    if kind == "adam":
        c["m0"][-1] = MARKER["m"]
    c["marker"] = True
    return c


def p_start_marked(c, which):
    p = p_start(c, which)
    if c.get("marker") and which == "randn":
        p[-1] = MARKER["p"]
    return p


def cu_sizes(cus):
    """The last count on the in-kernel norm hand-off and the first on norm_partials_kernel."""
    return (OCHUNK * cus, OCHUNK * cus + 1)


# ---------------------------------------------------------------------------------------
# cached references and error measures
# ---------------------------------------------------------------------------------------
_REFS = {}


def _args(c, which):
    return (c["kind"], p_start_marked(c, which), c["g"], c["m0"], c["v0"], c["t0"], c["hyper"],
            c["max_norm"])


def refs(c, which):
    """(step_ref, step_f32, terr) of a case from one parameter start, computed once and left
    unchanged; terr is the f32 formulation's update error from the zero start."""
    key = (c["name"], which)
    if key not in _REFS:
        r, f = step_ref(*_args(c, which)), step_f32(*_args(c, which))
        if which == "zero":
            terr = update_err(f["p"], r, skip=overflow_mask(c))
        else:
            terr = refs(c, "zero")[2]
        _REFS[key] = (r, f, terr)
    return _REFS[key]


def double_hyper_deviation(c, p_got=None):
    """Largest relative deviation of an update (the f32-hyperparameter reference's, or a
    zero-start run's p_got) from the reference on Python-double hyperparameters -- what
    torch's fused Adam computes.  Reported, never asserted."""
    rd = step_ref(*_args(c, "zero"), double_hyper=True)
    if p_got is None:
        p_got = -refs(c, "zero")[0]["update"]
    return update_err(p_got, rd, skip=overflow_mask(c))


def overflow_mask(c):
    """The elements of the overflow case whose f32 second moment is inf where f64's is not
    (None for every other case)."""
    if c["floor"]:
        return None
    mask = np.zeros(c["n"], bool)
    mask[list(OVERFLOW_POS_1E21)] = True
    return mask


def update_err(p_got, ref, skip=None):
    """Largest elementwise relative error of the update from a zero start (p_new = -update).
    Non-finite reference updates must be met in kind (NaN where NaN), an exactly-zero one
    exactly; no non-zero reference update is so small that f32 could not hold it to full
    precision."""
    got, want = -np.asarray(p_got, np.float64), ref["update"]
    keep = np.ones(len(want), bool) if skip is None else ~skip
    got, want = got[keep], want[keep]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert fin[~np.isnan(want)].all(), "an infinite reference update"
    zero = fin & (want == 0.0)
    assert (got[zero] == 0.0).all(), "a zero update came back non-zero"
    nz = fin & ~zero
    if not nz.any():
        return 0.0
    assert np.abs(want[nz]).min() > 2.0 ** -120
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))


@functools.lru_cache(maxsize=None)
def floor():
    """The largest terr over the cases that count: every fixed-size case (the sizes
    included) but the overflow one."""
    worst = 0.0
    for kind in KINDS:
        cs = regime_cases(kind) + [case_size(kind, n, mn) for n in SIZES for mn in (None, 0.5)]
        for c in cs:
            assert c["floor"]
            worst = max(worst, refs(c, "zero")[2])
    return worst


def update_bound(terr):
    return max(4.0 * terr, floor())


def k_moments(c):
    """(K_M, K_V) of the module docstring."""
    return (8, 12) if c["max_norm"] else (6, 8)


def same_nonfinite(got, want, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    inf = np.isinf(want)
    np.testing.assert_array_equal(np.asarray(got, np.float64)[inf], want[inf], err_msg=what)
    assert np.isfinite(np.asarray(got)[np.isfinite(want)]).all(), what


def moment_err(got, want, terms, k, subnormal_zero):
    """Largest |got - want| in units of k u terms + k eta over the finite entries; non-finite
    ones must match in kind.  subnormal_zero: an entry whose reference is below 2^-126 may be
    exactly 0 instead."""
    same_nonfinite(got, want, "moment")
    fin = np.isfinite(want)
    got, want, terms = np.asarray(got, np.float64)[fin], want[fin], terms[fin]
    e = np.abs(got - want) / (k * U * terms * (1 + 1e-6) + k * ETA)
    if subnormal_zero:
        e[(np.abs(want) < TINY) & (got == 0.0)] = 0.0
    return float(e.max()) if e.size else 0.0


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


def ulps_apart(a, b):
    """Distance of two finite f32 values of one sign in units in the last place."""
    ia, ib = (int(np.array(x, F32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


def check_clip(c, norm_out, ref):
    """norm_out[0] within 1 ulp of the rounded exact norm, norm_out[1] within 2 ulp of the
    reference coefficient and exactly 1.0 where that clamps; NaN / inf met in kind."""
    norm, coef = ref["norm"], ref["coef"]
    for got, want, ulps in ((norm_out[0], norm, 1), (norm_out[1], coef, 2)):
        if np.isfinite(want):
            assert np.isfinite(got) and ulps_apart(got, want) <= ulps, (c["name"], got, want)
        else:
            assert np.isnan(got) if np.isnan(want) else got == want, (c["name"], got, want)
    if coef == F32(1.0):
        assert norm_out[1] == F32(1.0), c["name"]


def check_outputs(c, which, got, skip=None):
    """got = dict(p, m, v) of one step of case c from the parameter start ``which``, against
    step_ref under the bounds of the module docstring.  skip: elements held to another
    expectation by the caller (the overflow positions).  Returns dict(err, terr, m, v, p):
    err / terr the update's relative error (zero start only), m / v / p the largest error in
    units of their bounds."""
    ref, _, terr = refs(c, which)
    keep = np.ones(c["n"], bool) if skip is None else ~skip
    km, kv = k_moments(c)
    out = dict(terr=terr, err=0.0, m=0.0, p=0.0)
    if c["kind"] == "adam":
        out["m"] = moment_err(got["m"][keep], ref["m"][keep], ref["m_terms"][keep], km, False)
    out["v"] = moment_err(got["v"][keep], ref["v"][keep], ref["v_terms"][keep], kv, True)
    bound = update_bound(terr)
    if which == "zero":
        out["err"] = update_err(got["p"], ref, skip)
        assert out["err"] <= bound, (c["name"], out["err"], terr, floor())
    else:
        gp, rp, upd = got["p"][keep], ref["p"][keep], ref["update"][keep]
        same_nonfinite(gp, rp, c["name"] + " p")
        fin = np.isfinite(rp)
        e = np.abs(gp[fin].astype(np.float64) - rp[fin]) / (ulp32(rp[fin])
                                                            + bound * np.abs(upd[fin]))
        out["p"] = float(e.max()) if e.size else 0.0
    assert max(out["m"], out["v"], out["p"]) <= 1.0, (c["name"], which, out)
    return out


def report(c, which, figs, extra=""):
    print(f"OPTIM-EDGES {c['name']} [{which}]: err {figs['err']:.3g} terr {figs['terr']:.3g} "
          f"floor {floor():.3g} m {figs['m']:.3g} v {figs['v']:.3g} p {figs['p']:.3g}{extra}")
