"""tsrl_clip_adam / tsrl_clip_rmsprop (csrc/optim.hip) called directly through the C ABI, so
that step, nstep, lr_dev, eps, the betas and a zero parameter vector are the test's to set,
against the f64 reference of tests/optim_edges_common.py (anchored to torch's own f64
optimisers by tests/test_optim_edges_host.py) under the derived bounds stated there: m and v
within K u sum|terms|, the update's relative error within max(4 terr, floor) of the f32
formulation's own, norm_out within 1 / 2 ulp.  p, g, m, v, the step words, norm_out and the
tickets are slices of larger buffers with 16 guard words on each side, checked after every
launch.

Measured on an MI355X (profiles/optim_edges_gpu_tests.log), nothing failing on the kernels'
arithmetic.  The update: Adam err up to 4.7e-7 against terr up to 4.4e-7, and at t = 2 err
3.63e-6 against terr 3.65e-6 (the cancellation in 1 - beta2^t, which sets the floor, 3.65e-6);
RMSprop err up to 2.5e-7 against terr up to 2.7e-7; the largest err / bound is 0.25.  m up to
0.24 and v up to 0.24 of their bounds; p of the N(0,1) start 0.50 of its bound (half an f32
ulp).  norm_out within 1 / 2 ulp everywhere.  Against Python-double hyperparameters (torch's
fused Adam) the kernel's Adam update deviates by 2.5e-7 at t = 1, 7.5e-6 at t = 2, 6.4e-6 at
t = 10, 3.9e-6 at t = 1000 and 2.5e-7 at t = 100 000 (beta2 reaches the kernel rounded to f32),
under 3e-9 of a parameter per step at lr 3e-4; RMSprop's by up to 6.1e-7.
"""
import numpy as np
import pytest
import torch

from . import optim_edges_common as oc

pytestmark = pytest.mark.gpu

GUARD = 16
SENT = {torch.float32: (torch.int32, 0xFFC0DE01 - (1 << 32)),
        torch.int32: (torch.int32, 0x5EC0DE01),
        torch.float64: (torch.int64, 0xFFF8C0DE0000BEEF - (1 << 64))}
STARTS = ("zero", "randn")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """An array inside a sentinel-filled buffer, 16 guard words on each side."""

    def __init__(self, dev, a, dtype=torch.float32):
        it, self.sent = SENT[dtype]
        src = torch.from_numpy(np.ascontiguousarray(a))
        assert src.dtype == dtype
        n = len(a)
        self.ibuf = torch.full((n + 2 * GUARD,), self.sent, dtype=it, device=dev)
        self.lo, self.hi = GUARD, GUARD + n
        self.t = self.ibuf.view(dtype)[self.lo:self.hi]
        self.t.copy_(src)

    def check(self, what=""):
        b = self.ibuf.cpu().numpy()
        assert (b[:self.lo] == self.sent).all() and (b[self.hi:] == self.sent).all(), \
            f"{what}: guard words overwritten"

    def numpy(self):
        return self.t.cpu().numpy()


class Bufs:
    """The device arguments of one parameter vector: p, g, m (Adam), v, nstep step words set
    to t0, norm_out[2], the slice partials, ticket[3] (zeroed once, as FlatAdam does)."""

    def __init__(self, dev, c, which, nstep=1):
        from tianshou_amd import _C
        self.c, self.dev, self.nstep = c, dev, nstep
        self.p = Guarded(dev, oc.p_start_marked(c, which))
        self.g = Guarded(dev, c["g"])
        self.m = Guarded(dev, c["m0"]) if c["kind"] == "adam" else None
        self.v = Guarded(dev, c["v0"])
        self.step = Guarded(dev, np.full(nstep, c["t0"], np.float32))
        self.norm = Guarded(dev, np.zeros(2, np.float32))
        nparts = max(int(_C.lib().tsrl_clip_adam_partials(c["n"])), 1)
        assert nparts == max((c["n"] + oc.OCHUNK - 1) // oc.OCHUNK, 1)
        self.partials = Guarded(dev, np.zeros(nparts, np.float64), torch.float64)
        self.ticket = Guarded(dev, np.zeros(3, np.int32), torch.int32)

    def all(self):
        return [x for x in (self.p, self.g, self.m, self.v, self.step, self.norm, self.partials,
                            self.ticket) if x is not None]

    def launch(self, lr_dev=None, scale_grads=1, max_norm="case", n=None, nstep=None, null=(),
               split=None, **hyper):
        """One call; returns its return code.  null: names of pointers passed as NULL."""
        from tianshou_amd import _C
        c = self.c
        h = dict(c["hyper"], **hyper)
        mn = c["max_norm"] if max_norm == "case" else max_norm
        P = lambda name: None if name in null else _C.ptr(getattr(self, name).t)  # noqa: E731
        head = [P("p"), P("g")] + ([P("m")] if c["kind"] == "adam" else []) + \
            [P("v"), c["n"] if n is None else n, P("step"), self.nstep if nstep is None else nstep,
             float(h["lr"])]
        mid = [h["beta1"], h["beta2"]] if c["kind"] == "adam" else [h["alpha"]]
        tail = [float(h["eps"]), float(mn) if mn else 0.0, P("partials"), P("norm"), P("ticket"),
                _C.ptr(lr_dev), split, int(scale_grads), _C.stream_ptr(self.dev)]
        fn = _C.lib().tsrl_clip_adam if c["kind"] == "adam" else _C.lib().tsrl_clip_rmsprop
        return fn(*head, *[float(x) for x in mid], *tail)

    def read(self, what=""):
        """Synchronise, check every guard, the step words and the tickets; the outputs."""
        torch.cuda.synchronize()
        for x in self.all():
            x.check(what or self.c["name"])
        out = dict(p=self.p.numpy(), g=self.g.numpy(), v=self.v.numpy(),
                   m=self.m.numpy() if self.m else None, step=self.step.numpy(),
                   norm=self.norm.numpy(), ticket=self.ticket.numpy())
        assert (out["ticket"] == 0).all(), (what, out["ticket"])
        return out


def _same_bits(a, b):
    """The same f32 bits, a NaN for a NaN (its sign and payload are the hardware's choice)."""
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and \
        np.array_equal(a.view(np.int32)[~nan], b.view(np.int32)[~nan])


def run_case(dev, c, which, **kw):
    """One launch of case c from the parameter start ``which``: return code 0, every step word
    t0 + 1, tickets 0, guards intact."""
    from tianshou_amd import _C
    b = Bufs(dev, c, which, kw.pop("nstep", 1))
    _C.check(b.launch(**kw), c["name"])
    out = b.read()
    assert (out["step"] == c["t0"] + 1).all(), (c["name"], out["step"])
    return out


def check_case(dev, c, skip=None, report=True):
    """Case c from both parameter starts through check_outputs / check_clip; with scaling the
    gradient afterwards is bit for bit g * norm_out[1].  Returns the zero start's figures."""
    figs0 = None
    for which in STARTS:
        out = run_case(dev, c, which)
        if c["max_norm"]:
            oc.check_clip(c, out["norm"], oc.refs(c, which)[0])
            with np.errstate(all="ignore"):
                want_g = c["g"] * out["norm"][1]
            assert _same_bits(out["g"], want_g), c["name"]
        else:
            assert out["g"].tobytes() == c["g"].tobytes(), c["name"]
        figs = oc.check_outputs(c, which, out, skip=skip)
        extra = ""
        if which == "zero" and "plain" in c["name"]:
            extra = f" double-hyper deviation {oc.double_hyper_deviation(c, out['p']):.3g}"
        if which == "zero" and "1e25" in c["name"]:
            tnorm, nonzero = oc.torch_f32_clip(c["g"], c["max_norm"])
            extra = (f"; kernel norm {out['norm'][0]:.6g} coef {out['norm'][1]:.6g}, torch f32 "
                     f"clip_grad_norm_ norm {tnorm:g} with {nonzero} non-zero gradients left")
        if report:
            oc.report(c, which, figs, extra)
        figs0 = figs0 or figs
    return figs0


# ---------------------------------------------------------------------------------------
# the regimes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["plain", "eps", "zeros", "tiny", "huge", "inf", "norm_edges"])
@pytest.mark.parametrize("kind", oc.KINDS)
def test_regimes_against_f64(dev, kind, group):
    """plain (g ~ N(0,1) {1e-4, 1, 1e4}, t0 in {0, 1, 9, 999, 99 999}), eps-dominated and
    mixed, zero gradients, denormal squares, 1e18 unclipped and 1e25 clipped, +-inf elements
    with and without clipping, the norm edges: every case from a zero and an N(0,1) parameter
    start.  The 1e25 case pins that the kernel, summing squares in f64, clips where torch's f32
    clip_grad_norm_ sees an inf norm and zeroes the step: the kernel is the more faithful.  An
    all-zero gradient moves nothing, bit for bit.  Measured, largest err / bound per group:
    Adam plain 0.25, eps 0.055, zeros 0.071, tiny 0.044, huge 0.11, inf 0.11, norm edges 0.11;
    RMSprop 0.059, 0.038, 0, 0.027, 0.054, 0.050, 0.055.  The 1e25 case: kernel norm 6.1938e26,
    coefficient 8.07258e-28, err 3.9e-7; torch's f32 clip_grad_norm_: norm inf, no non-zero
    gradient left."""
    worst = 0.0
    for c in getattr(oc, "cases_" + group)(kind):
        figs = check_case(dev, c)
        worst = max(worst, figs["err"] / oc.update_bound(figs["terr"]))
        if "all-zero" in c["name"]:
            for which in STARTS:
                out = run_case(dev, c, which)
                assert out["p"].tobytes() == oc.p_start(c, which).tobytes()
                assert not out["v"].any() and (out["m"] is None or not out["m"].any())
    print(f"OPTIM-EDGES {kind} {group}: largest err / bound {worst:.3g}")


@pytest.mark.parametrize("kind", oc.KINDS)
def test_overflow_follows_the_f32_formulation(dev, kind):
    """|g| = 1e20 and 1e21 unclipped: at 1e20 ((1-b2) g) g is finite in f32 and every output is
    held to the normal bounds; at 1e21 it is inf where f64's is finite, and the kernel does
    what step_f32 does: v = inf, m finite, an update of exactly 0 -- and v stays at inf through
    an ordinary second step.  Everywhere else the normal bounds.  Measured: err 2.3e-7 (Adam),
    1.6e-7 (RMSprop) over the elements that are compared."""
    from tianshou_amd import _C
    c = oc.case_overflow(kind)
    mask = oc.overflow_mask(c)
    check_case(dev, c, skip=mask)
    b = Bufs(dev, c, "randn")
    _C.check(b.launch(), c["name"])
    one = b.read()
    f = oc.refs(c, "randn")[1]
    assert np.isinf(one["v"][mask]).all() and (one["v"][mask] > 0).all()
    assert np.array_equal(np.isinf(one["v"]), np.isinf(f["v"]))
    assert one["p"][mask].tobytes() == f["p"][mask].tobytes()
    assert one["p"][mask].tobytes() == oc.p_start(c, "randn")[mask].tobytes()
    b.g.t.copy_(torch.from_numpy(oc.overflow_second_gradient()))
    _C.check(b.launch(), c["name"])
    two = b.read()
    assert (two["step"] == 2).all()
    assert np.isinf(two["v"][mask]).all() and np.isfinite(two["v"][~mask]).all()
    assert two["p"][mask].tobytes() == one["p"][mask].tobytes()
    assert np.isfinite(two["p"]).all()
    # (the ordinary elements step on; at |g| = 1e20 the second update is below an ulp of p)
    assert np.mean(two["p"][~mask] != one["p"][~mask]) > 0.99


# ---------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [None, 0.5])
@pytest.mark.parametrize("kind", oc.KINDS)
def test_sizes(dev, kind, max_norm):
    """n in {1, 255, 256, 257, 2047, 2048, 2049, 4097} (thread, wave-group and slice edges),
    {262 143, 262 144, 262 145} (one trip of clip_scale_kernel's grid and the first element of
    its second) and {2048 CUs, 2048 CUs + 1} (the last count on the in-kernel norm hand-off,
    the first on norm_partials_kernel), Adam and RMSprop, with a marker in the last element and
    guard words behind every buffer.  Measured, largest err / bound: Adam 0.12 unclipped, 0.13
    clipped (err up to 4.7e-7); RMSprop 0.063, 0.069 (err up to 2.5e-7)."""
    worst = 0.0
    for n in oc.SIZES + oc.cu_sizes(_cus()):
        c = oc.case_size(kind, n, max_norm)
        figs = check_case(dev, c)
        worst = max(worst, figs["err"] / oc.update_bound(figs["terr"]))
    print(f"OPTIM-EDGES {kind} sizes max_norm={max_norm}: largest err / bound {worst:.3g}")


def test_cu_edge_is_where_the_norm_launch_takes_over(dev):
    """The CU count the sizes use is the one tsrl's host code reads: 2048 * CUs elements are
    CUs slices, one more element is CUs + 1."""
    from tianshou_amd import _C
    lo, hi = oc.cu_sizes(_cus())
    assert int(_C.lib().tsrl_clip_adam_partials(lo)) == _cus()
    assert int(_C.lib().tsrl_clip_adam_partials(hi)) == _cus() + 1


# ---------------------------------------------------------------------------------------
# the ABI surface FlatAdam drives one way
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", oc.KINDS)
def test_step_words_and_start(dev, kind):
    """nstep in {1, 3, 12}: every word is t0 + 1 afterwards (t0 = 999, a non-zero start), the
    words behind them untouched, and the outputs are the bits of the nstep = 1 run."""
    c = oc.case_size(kind, 4097, 0.5)
    c = dict(c, t0=999, name=c["name"] + " t0=999")
    base = run_case(dev, c, "randn")
    oc.check_outputs(c, "randn", base)
    for nstep in (3, 12):
        out = run_case(dev, c, "randn", nstep=nstep)
        assert len(out["step"]) == nstep
        for k in ("p", "m", "v", "g", "norm"):
            if out[k] is not None:
                assert out[k].tobytes() == base[k].tobytes(), (nstep, k)


@pytest.mark.parametrize("kind", oc.KINDS)
def test_lr_word(dev, kind):
    """A device lr word different from the host lr wins; nullptr takes the host lr."""
    c = oc.case_size(kind, 2049, None)
    lr = c["hyper"]["lr"]
    word = torch.tensor([lr], dtype=torch.float32, device=dev)
    host = run_case(dev, c, "randn")
    oc.check_outputs(c, "randn", host)
    assert run_case(dev, c, "randn", lr_dev=word, lr=lr * 10)["p"].tobytes() == host["p"].tobytes()
    assert run_case(dev, c, "randn", lr=lr * 10)["p"].tobytes() != host["p"].tobytes()
    c10 = dict(c, hyper=dict(c["hyper"], lr=lr * 10), name=c["name"] + " lr x10")
    oc.check_outputs(c10, "randn", run_case(dev, c10, "randn", lr_dev=None))
    word.fill_(lr * 10)
    oc.check_outputs(c10, "randn", run_case(dev, c, "randn", lr_dev=word))


@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("n", [4097, oc.SCALE_SPAN + 1])
def test_scale_grads(dev, kind, n):
    """scale_grads 1: the gradient afterwards is bit for bit g * norm_out[1], one f32 multiply
    by the kernel's own coefficient (past one trip of clip_scale_kernel's grid too); 0: the
    gradient keeps its bits; p, m, v are the same bits either way."""
    c = oc.case_size(kind, n, 0.5)
    on, off = run_case(dev, c, "randn", scale_grads=1), run_case(dev, c, "randn", scale_grads=0)
    assert 0 < on["norm"][1] < 1
    assert on["g"].tobytes() == (c["g"] * on["norm"][1]).tobytes()
    assert off["g"].tobytes() == c["g"].tobytes()
    for k in ("p", "m", "v", "norm"):
        if on[k] is not None:
            assert on[k].tobytes() == off[k].tobytes(), k


@pytest.mark.parametrize("kind", oc.KINDS)
def test_handoff_run_is_deterministic(dev, kind):
    """Two runs of the n = 2048 CUs clipped case (every slice on the in-kernel hand-off) give
    identical bits."""
    c = oc.case_size(kind, oc.cu_sizes(_cus())[0], 0.5)
    a, b = run_case(dev, c, "randn"), run_case(dev, c, "randn")
    for k in ("p", "m", "v", "g", "norm"):
        if a[k] is not None:
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("kind", oc.KINDS)
def test_back_to_back_launches(dev, kind):
    """20 launches on one stream with no host synchronisation between them (what a captured
    epoch does; the gradient rescaled in place by each) give the bits of 20 synchronised ones;
    afterwards the step is t0 + 20 and the tickets -- the sticky hand-off word ticket[2]
    FlatAdam.check_handoff reads included -- are 0."""
    from tianshou_amd import _C
    c = oc.case_size(kind, 57763, 0.5)
    runs = []
    for sync in (True, False):
        b = Bufs(dev, c, "randn", nstep=3)
        for _ in range(20):
            _C.check(b.launch(), c["name"])
            if sync:
                torch.cuda.synchronize()
                assert (b.ticket.numpy() == 0).all()
        out = b.read()  # asserts the tickets are 0
        assert (out["step"] == c["t0"] + 20).all()
        assert np.isfinite(out["p"]).all()
        runs.append(out)
    for k in ("p", "m", "v", "g", "norm"):
        if runs[0][k] is not None:
            assert runs[0][k].tobytes() == runs[1][k].tobytes(), k


@pytest.mark.parametrize("n", [4097, "cus+1"])
@pytest.mark.parametrize("kind", oc.KINDS)
def test_refusals(dev, kind, n):
    """n < 0, nstep < 1, a null pointer, clipping without norm_out / partials, a split range
    past n: each returns an error that names the entry, launches nothing (every buffer keeps
    its bits, the slice partials included) and leaves step unchanged; n == 0 returns 0 and
    changes nothing; the same arguments unbroken are accepted.  At 2048 CUs + 1 elements the
    first launch would be norm_partials_kernel: the split check used to come after it, which
    this test found; every check precedes it now."""
    from tianshou_amd import _C
    c = oc.case_size(kind, oc.cu_sizes(_cus())[1] if n == "cus+1" else n, 0.5)
    b = Bufs(dev, c, "randn", nstep=3)
    before = [x.ibuf.clone() for x in b.all()]
    entry = "tsrl_clip_adam" if kind == "adam" else "tsrl_clip_rmsprop"

    def unchanged(what):
        torch.cuda.synchronize()
        for k, x in enumerate(b.all()):
            assert torch.equal(x.ibuf, before[k]), (what, k)

    out = torch.zeros(6 * 128 * 32, dtype=torch.bfloat16, device=dev)
    past = _C.W1Split(_C.ptr(out), 0, c["n"] - 64 * 17 + 1, 17, 32)
    bad = {"n < 0": dict(n=-1), "nstep < 1": dict(nstep=0),
           "clip without norm_out": dict(null=("norm",)),
           "clip without partials": dict(null=("partials",)),
           "split past n": dict(split=past)}
    nulls = ("p", "g", "v", "step", "ticket") + (("m",) if kind == "adam" else ())
    bad.update({f"null {k}": dict(null=(k,)) for k in nulls})
    for what, kw in bad.items():
        rc = b.launch(**kw)
        assert rc != 0, what
        msg = _C.lib().tsrl_last_error().decode(errors="replace")
        assert entry + ":" in msg, (what, msg)
        unchanged(what)
    assert b.launch(n=0) == 0
    assert b.launch(n=0, null=("p", "g", "m", "v", "step", "ticket", "norm", "partials")) == 0
    unchanged("n == 0")
    _C.check(b.launch(), "accepted")
    assert (b.read()["step"] == c["t0"] + 1).all()


# ---------------------------------------------------------------------------------------
# through FlatAdam
# ---------------------------------------------------------------------------------------
def _flat_pair(kind, n, seed):
    """test_gpu_rmsprop.py's _flat_pair for either optimiser."""
    from tianshou_amd.policy.flat_adam import FlatAdam
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    sizes = [n] if n == 1 else [n // 3, n - n // 3]
    p0 = [torch.nn.Parameter(torch.randn(k, device=dev, generator=g)) for k in sizes]
    p1 = [torch.nn.Parameter(p.detach().clone()) for p in p0]
    make = (lambda ps: torch.optim.Adam(ps, lr=3e-4)) if kind == "adam" else \
        (lambda ps: torch.optim.RMSprop(ps, lr=7e-4, eps=1e-5, alpha=0.99))
    opt_ref, opt = make(p0), make(p1)
    fa = FlatAdam(p1)
    assert fa.bind_adam(opt) and fa.adam_bound(opt)
    return p0, p1, opt_ref, opt, fa, g


@pytest.mark.parametrize("max_norm", [0.5, None, 1e3])
@pytest.mark.parametrize("n", [1, 2047, 2049, 57763, "cus"])
def test_flat_adam_matches_torch_at_slice_edges(n, max_norm):
    """test_gpu_rmsprop.py::test_clip_rmsprop_matches_torch's sizes for Adam, at its
    tolerances (torch's f32 optimiser is the reference here: parameters rtol 1e-5 / atol 1e-7,
    clipped gradients rtol 1e-5 / atol 1e-9, the norm rtol 5e-5), with exp_avg_sq at
    test_gpu_optim.py's rtol 5e-5 and exp_avg at a derived absolute bound after every step."""
    n = 2048 * _cus() + 5 if n == "cus" else n
    dev = torch.device("cuda", 0)
    p0, p1, opt_ref, opt, fa, g = _flat_pair("adam", n, 1)
    gmax = 0.0  # the largest (clipped) gradient element over the steps
    for step in range(4):
        scale = 10.0 ** (step % 3 - 1)
        grads = [torch.randn(p.shape, device=dev, generator=g) * scale for p in p0]
        for p, gr in zip(p0, grads):
            p.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_(p0, max_norm=max_norm) if max_norm else None
        opt_ref.step()
        gmax = max([gmax] + [float(p.grad.abs().max()) for p in p0])
        fa.bind_grads()
        for p, gr in zip(p1, grads):
            p.grad.copy_(gr)
        fa.clip_adam(max_norm)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(p0, p1)):
            np.testing.assert_allclose(b.detach().cpu().numpy(), a.detach().cpu().numpy(),
                                       rtol=1e-5, atol=1e-7, err_msg=f"step {step} param {i}")
            np.testing.assert_allclose(b.grad.cpu().numpy(), a.grad.cpu().numpy(), rtol=1e-5,
                                       atol=1e-9, err_msg=f"grad step {step} param {i}")
            # torch forms 1 - beta2 in double (0.001), the kernel from the f32 beta2
            # (0.00099998713): up to 2^-25 beta2 / (1 - beta2) = 3.0e-5 relative in a young
            # exp_avg_sq (1.3e-5 measured), on top of the 1e-5 of f32 roundoff; 5e-5 / 1e-12 is
            # test_gpu_optim.py's tolerance for it
            np.testing.assert_allclose(opt.state[b]["exp_avg_sq"].cpu().numpy(),
                                       opt_ref.state[a]["exp_avg_sq"].cpu().numpy(), rtol=5e-5,
                                       atol=1e-12, err_msg=f"exp_avg_sq step {step} param {i}")
            # exp_avg sums terms of either sign: the absolute bound 2^-17 max |g| derived in
            # test_gpu_optim.py::test_clip_adam_matches_torch
            np.testing.assert_allclose(opt.state[b]["exp_avg"].cpu().numpy(),
                                       opt_ref.state[a]["exp_avg"].cpu().numpy(), rtol=0,
                                       atol=2.0 ** -17 * gmax,
                                       err_msg=f"exp_avg step {step} param {i}")
        if max_norm:
            np.testing.assert_allclose(float(fa._adam["norm"][0]), float(norm), rtol=5e-5)
    for a, b in zip(p0, p1):
        assert float(opt.state[b]["step"]) == float(opt_ref.state[a]["step"]) == 4.0
        assert set(opt.state[b]) == {"step", "exp_avg", "exp_avg_sq"}
    fa.check_handoff()
