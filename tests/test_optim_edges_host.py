"""The cases and references of tests/test_gpu_optim_edges.py checked on the CPU: every case
of tests/optim_edges_common.py is what it claims to be (eps-dominated, denormal, finite or
overflowing in f32, on the stated side of the clamp); ``step_ref`` agrees with torch's own
Adam / RMSprop run at float64; the f32 formulation ``step_f32`` stays inside every bound the
GPU file applies to the kernel, so the bounds are passable before a GPU is involved; and the
only elements excused from a comparison are the constructed ones.

Figures of this file's ``-s`` output: the floor (the largest terr) is 3.65e-6, set by Adam at
t = 2 (the cancellation in 1 - beta2^t; 3.60e-6 to 3.65e-6 over the three gradient scales);
elsewhere terr is 1.0e-7 to 4.8e-7 for Adam and 1.0e-7 to 2.7e-7 for RMSprop (less at n = 1).
The f64 reference on f32-rounded hyperparameters deviates from Python-double hyperparameters
(torch's fused Adam) by 4.9e-8 of the update at t = 1 (lr / (1 - b1) meets (1 - b1) g), 3.95e-6
at t = 2, 6.06e-6 at t = 10, 3.71e-6 at t = 1000 and 7.5e-8 at t = 100 000 (beta2 = 0.999
reaches the kernel as 0.99900001287), under 2e-9 of a parameter per step at lr 3e-4; RMSprop
by up to 4.4e-7 (alpha = 0.99 as 0.99000000954).
"""
import numpy as np
import pytest
import torch

from . import optim_edges_common as oc

STARTS = ("zero", "randn")


def _all_fixed_cases(kind):
    return (oc.regime_cases(kind) + [oc.case_overflow(kind)]
            + [oc.case_size(kind, n, mn) for n in oc.SIZES for mn in (None, 0.5)])


@pytest.mark.parametrize("kind", oc.KINDS)
def test_eps_cases_are_eps_dominated(kind):
    """sqrt(v_hat) < eps on every element of the eps-dominated cases; on a share inside
    MIXED_SHARE of the mixed Adam case (measured 0.87 at t0 0, 0.84 at t0 999)."""
    for c in oc.cases_eps(kind):
        eps = oc.as_f32(c["hyper"])["eps"]
        share = float(np.mean(oc.sqrt_vhat(c) < eps))
        print(f"OPTIM-EDGES {c['name']}: share of sqrt(v_hat) < eps {share:.3f}")
        if "mixed" in c["name"]:
            assert oc.MIXED_SHARE[0] < share < oc.MIXED_SHARE[1], c["name"]
        else:
            assert share == 1.0, c["name"]
    assert any("mixed" in c["name"] for c in oc.cases_eps("adam"))


@pytest.mark.parametrize("kind", oc.KINDS)
def test_tiny_and_huge_are_where_they_claim(kind):
    """tiny: every f32 square is below the smallest normal and over 99 % are non-zero
    denormals.  huge 1e18: g g and ((1-b2) g) g are finite in f32 on every element.  huge
    1e25: over 99 % of the f32 squares are inf while the exact norm is finite in f32; torch's
    f32 clip_grad_norm_ of the same gradient is printed."""
    with np.errstate(all="ignore"):
        for c in oc.cases_tiny(kind):
            sq = c["g"] * c["g"]
            assert sq.dtype == np.float32 and (sq < oc.TINY).all()
            assert np.mean(sq > 0) > 0.99
        unclipped, clipped = oc.cases_huge(kind)
        g = unclipped["g"]
        assert np.isfinite(g * g).all() and np.abs(g).max() > 3e18
        assert np.isfinite(oc.step_f32(*oc._args(unclipped, "zero"))["v"]).all()
        g = clipped["g"]
        assert np.mean(np.isinf(g * g)) > 0.99
    norm = oc.exact_norm(g)
    assert np.isfinite(np.float32(norm)) and norm > 1e26
    tnorm, nonzero = oc.torch_f32_clip(g, 0.5)
    print(f"OPTIM-EDGES {clipped['name']}: exact norm {norm:.6g}; torch f32 clip_grad_norm_ "
          f"norm {tnorm:g} with {nonzero} non-zero gradients left")


@pytest.mark.parametrize("kind", oc.KINDS)
def test_norm_edges_land_on_their_side(kind):
    """Under math.fsum the scaled gradients have the stated exact norm to 1e-8 relative (the
    distance to the clamp is 2^-20 ~ 9.5e-7), and the f32 coefficient clamps exactly where
    NORM_EDGES says; the all-zero gradient clamps; max_norm 1e30 clamps, 1e-30 does not."""
    cs = {c["name"]: c for c in oc.cases_norm_edges(kind)}
    for name, max_norm, target, clamps in oc.NORM_EDGES:
        c = cs[f"{kind} {name}"]
        assert abs(oc.exact_norm(c["g"]) / target - 1.0) < 1e-8
        coef = oc.clip_ref(c["g"], max_norm)[1]
        assert (coef == np.float32(1.0)) == clamps, (name, coef)
        if not clamps:
            assert coef < np.float32(1.0)
    assert oc.clip_ref(cs[f"{kind} norm all-zero clipped"]["g"], 0.5) == (0.0, 1.0)
    assert oc.clip_ref(cs[f"{kind} max_norm=1e+30"]["g"], 1e30)[1] == 1.0
    assert 0 < oc.clip_ref(cs[f"{kind} max_norm=1e-30"]["g"], 1e-30)[1] < 1e-30


@pytest.mark.parametrize("kind", oc.KINDS)
def test_step_ref_equals_torch_f64(kind):
    """step_ref against torch.optim.Adam / RMSprop at float64 on the CPU from the same state,
    with the f32-rounded hyperparameters, on the plain cases: 1e-12 relative."""
    for c in oc.cases_plain(kind):
        h = oc.as_f32(c["hyper"])
        p = torch.nn.Parameter(torch.from_numpy(oc.p_start(c, "randn").astype(np.float64)))
        p.grad = torch.from_numpy(c["g"].astype(np.float64))
        state = dict(step=torch.tensor(float(c["t0"])))
        if kind == "adam":
            opt = torch.optim.Adam([p], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
            state.update(exp_avg=torch.from_numpy(c["m0"].astype(np.float64)),
                         exp_avg_sq=torch.from_numpy(c["v0"].astype(np.float64)))
        else:
            opt = torch.optim.RMSprop([p], lr=h["lr"], alpha=h["alpha"], eps=h["eps"])
            state.update(square_avg=torch.from_numpy(c["v0"].astype(np.float64)))
        if c["t0"]:
            opt.state[p] = state
        opt.step()
        ref = oc.refs(c, "randn")[0]
        st = opt.state[p]
        assert float(st["step"]) == c["t0"] + 1
        np.testing.assert_allclose(p.detach().numpy(), ref["p"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(st["exp_avg_sq" if kind == "adam" else "square_avg"].numpy(),
                                   ref["v"], rtol=1e-12, atol=0)
        if kind == "adam":
            np.testing.assert_allclose(st["exp_avg"].numpy(), ref["m"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_f32_formulation_is_inside_every_bound(kind):
    """step_f32 through the checks the GPU file applies to the kernel, on every fixed-size
    case from both parameter starts, and the clip coefficient of every clipped case: the
    reference's own f32 formulation passes.  Prints err (= terr here), the floor and the
    deviation from Python-double hyperparameters per case."""
    for c in _all_fixed_cases(kind):
        ref = oc.refs(c, "zero")[0]
        if c["max_norm"]:
            oc.check_clip(c, (ref["norm"], ref["coef"]), ref)
        for which in STARTS:
            f = oc.refs(c, which)[1]
            figs = oc.check_outputs(c, which, f, skip=oc.overflow_mask(c))
            extra = ""
            if which == "zero" and "plain" in c["name"]:
                extra = f" double-hyper deviation {oc.double_hyper_deviation(c):.3g}"
            oc.report(c, which, figs, extra)
            assert figs["err"] == (figs["terr"] if which == "zero" else 0.0)
    assert 1e-7 < oc.floor() < 2e-5  # (f32 roundoff is 6e-8; t = 2 costs up to 7.5e-6)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_only_constructed_elements_are_excused(kind):
    """The overflow positions -- f32 second moment inf where f64's is finite -- are exactly
    OVERFLOW_POS_1E21 (the |g| = 1e20 elements stay finite and fully compared), there the f32
    update is exactly 0 and a second step leaves v at inf; the denormal-or-zero allowance of v
    applies to the tiny and max_norm 1e-30 cases alone; every non-finite reference value is at
    a constructed inf element."""
    c = oc.case_overflow(kind)
    ref, f, _ = oc.refs(c, "randn")
    mask = oc.overflow_mask(c)
    assert np.array_equal(np.flatnonzero(np.isinf(f["v"]) & np.isfinite(ref["v"])),
                          sorted(oc.OVERFLOW_POS_1E21))
    assert np.isfinite(ref["v"]).all() and np.isfinite(f["v"][~mask]).all()
    assert np.array_equal(f["p"][mask], oc.p_start(c, "randn")[mask])
    f2 = oc.step_f32(kind, f["p"], oc.overflow_second_gradient(), f["m"], f["v"], 1, c["hyper"],
                     None)
    assert np.isinf(f2["v"][mask]).all() and np.isfinite(f2["v"][~mask]).all()
    assert np.array_equal(f2["p"][mask], f["p"][mask]) and np.isfinite(f2["p"]).all()
    for c in _all_fixed_cases(kind):
        ref = oc.refs(c, "zero")[0]
        sub = (ref["v"] > 0) & (ref["v"] < oc.TINY)
        if sub.any():
            assert "tiny" in c["name"] or "max_norm=1e-30" in c["name"], c["name"]
        bad = ~np.isfinite(ref["p"])
        assert np.array_equal(bad, ~np.isfinite(c["g"]) | (np.isnan(ref["coef"]) if
                                                           c["max_norm"] else False)), c["name"]
