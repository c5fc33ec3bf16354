"""The off-policy loss kernels (csrc/dsac.hip: tsrl_dsac_target, tsrl_dsac_actor_loss_fwd_bwd;
csrc/dqn_dist.hip: tsrl_c51_loss_fwd_bwd, tsrl_qr_loss_fwd_bwd, tsrl_dist_select) through their
wrappers, and through the C ABI for the argument errors, against the f64 references of
tests/offpolicy_edges_common.py, where tests/test_gpu_dsac.py and tests/test_gpu_dist_dqn.py do
not go: -inf (masked) logits in every position, finite extremes, rows poisoned by an all -inf
row, a +inf or a NaN logit, NaN and infinite returns, a NaN in the next distribution, and the
widths at which a thread owns several atoms (N = 255 .. 513), the limit N = 4096 and the
argument error above it.

Tolerance (tests/test_gpu_noisy.py's rule, as in tests/test_gpu_loss_edges.py): per output,
err = the kernel's error against f64 and terr = the torch-f32 formulation's, run on the device,
both scaled by max |ref|; floor = the largest terr over the case list (the two "extreme" cases,
whose f32 error is large by construction, do not raise it); err <= max(4 * terr, floor).  Every
case prints err, terr and floor.  Beside it: an output is NaN (or infinite) exactly where the
f64 reference is, rows a poison does not touch are bit for bit the clean run's, two launches
give the same bits, and the gradient is exactly 0 at a masked entry.

Measured on an MI355X (profiles/offpolicy_edges_gpu_tests.log), the largest err of an output
over its cases, with that case's terr and the floor: DiscreteSAC target 4.85e-8 / 6.76e-8 /
1.68e-7, actor loss 4.21e-8 / 4.21e-8 / 1.46e-7, temperature loss 4.35e-8 / 4.35e-8 / 1.67e-7,
g_logits 5.04e-8 / 3.63e-7 / 5.15e-6, g_log_alpha 4.57e-8 / 4.57e-8 / 1.52e-7; on the two extreme
cases the kernel stays at or below 4.01e-8 where torch f32 is 1.7e-5 .. 5.0e-5 off.  C51 loss
4.91e-8 / 5.79e-8 / 1.59e-7, cross-entropy 4.35e-8 / 1.52e-7 / 1.52e-7, gradient 4.74e-8 /
5.07e-8 / 1.51e-7; QR loss 5.53e-8 / 6.13e-8 / 1.93e-7, priority 4.92e-8 / 4.92e-8 / 1.24e-7,
gradient 5.04e-8 / 1.25e-7 / 1.79e-7.  The kernels sum in f64 and round once: err is one f32
rounding at every width, N = 4096 included; in no case is it above its terr.  tsrl_dist_select:
0 ulp from the rounded f64 value in every case.  The masked learn test: max |parameter - twin|
9.69e-8 after three updates.
"""
import copy

import numpy as np
import pytest
import torch

from tests import dsac_common
from tests import loss_edges_common as lc
from tests import offpolicy_edges_common as oc
from tests.test_gpu_ddpg import _bits
from tests.test_gpu_dist_dqn import _c51_kernel, _qr_kernel, _ulp
from tianshou_amd import _C
from tianshou_amd.policy.discrete_sac import dsac_actor_loss, dsac_target_device
from tianshou_amd.policy.dqn_dist import dist_select

pytestmark = pytest.mark.gpu

SENT = -777.0  # prefilled into outputs a refused call must not write


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def r32(dev):
    """r32(name): the torch-f32 formulation of a case evaluated on the device, once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oc.ref_of(name, torch.float32, dev)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def floor(r32):
    return oc.floors(oc.CASES, r32)


def run_dsac(dev, case):
    """The five outputs of oc.DSAC_OUTPUTS from one target launch and one actor-loss launch."""
    logits, q1, q2 = (case[k].to(dev).contiguous() for k in ("logits", "q1", "q2"))
    alpha = torch.full((1,), oc.ALPHA, device=dev)
    log_alpha = torch.full((1,), oc.LOG_ALPHA, device=dev)
    target = dsac_target_device(logits, q1, q2, alpha)
    x = logits.clone().requires_grad_(True)
    handle, loss, g_la = dsac_actor_loss(x, q1, q2, alpha, log_alpha, case["te"])
    handle.backward()
    return dict(target=target, loss=loss[0], alpha_loss=loss[1], g_logits=x.grad,
                g_log_alpha=g_la.reshape(()))


def run_dist(dev, case):
    args = oc.dist_args(case, torch.float32, dev)
    got = _c51_kernel(*args) if case["kind"] == "c51" else _qr_kernel(*args)
    return dict(zip(oc.DIST_OUTPUTS, got))


def run_case(dev, name):
    case = oc.CASES[name]
    return (run_dsac if case["kind"] == "dsac" else run_dist)(dev, case)


def same_bits(a, b):
    return all(torch.equal(_bits(a[o]), _bits(b[o])) for o in a)


def check_case(name, got, floor, r32):
    """err <= max(4 terr, floor) per output, and NaN / infinite exactly where f64 is."""
    case = oc.CASES[name]
    r64, t32 = oc.ref64(name), r32(name)
    bad = []
    for o in oc.outputs(case["kind"]):
        err = oc.case_err(case, got[o], r64[o], o)
        terr = oc.case_err(case, t32[o], r64[o], o)
        fl = floor.get((case["kind"], o), 0.0)
        print(f"{name} {o}: err {err:.2e} terr {terr:.2e} floor {fl:.2e}")
        g = got[o].detach().cpu()
        if not err <= max(4 * terr, fl) or not oc.same_nans(g, r64[o]) or \
                not torch.equal(torch.isinf(g), torch.isinf(r64[o])):
            bad.append((o, err, terr, fl, int(torch.isnan(g).sum()),
                        int(torch.isnan(r64[o]).sum())))
    assert not bad, bad


# -- DiscreteSAC: masked, extreme and poisoned rows ------------------------------------------------
@pytest.mark.parametrize("name", oc.names("masked") + oc.names("plain") + oc.names("extreme"))
def test_dsac_rows(dev, floor, r32, name):
    """-inf logits in every position, plain rows and finite extremes: everything finite, the
    gradient exactly 0 at every masked entry, values against f64, two launches the same bits."""
    case = oc.CASES[name]
    got = run_dsac(dev, case)
    masked = case["logits"] == -oc.INF
    g = got["g_logits"].cpu()
    print(f"{name}: {int(torch.isnan(g).sum())} NaN of {g.numel()} gradient entries, "
          f"{int(masked.sum())} masked; loss {float(got['loss']):.6g}")
    assert bool(torch.isfinite(g).all()), "non-finite g_logits"
    assert bool((g[masked] == 0).all()), "exactly 0 at masked entries"
    assert all(bool(torch.isfinite(got[o]).all()) for o in oc.DSAC_OUTPUTS)
    check_case(name, got, floor, r32)
    assert same_bits(got, run_dsac(dev, case))


@pytest.mark.parametrize("A", (6, 130))
@pytest.mark.parametrize("kind", oc.POISONS)
def test_dsac_poisoned_row_stays_contained(dev, floor, r32, kind, A):
    """A row of all -inf, with a +inf or with a NaN logit: NaN in that row's target and
    gradient and in the losses, as the reference; every other row bit for bit the clean
    run's."""
    name = f"poison-{kind}-A{A}"
    case = oc.CASES[name]
    got, clean = run_dsac(dev, case), run_dsac(dev, oc.CASES[f"clean-A{A}"])
    r64 = oc.ref64(name)
    keep = oc.clean_rows(case).to(dev)
    print(f"{name}: NaN rows of target {torch.isnan(got['target']).nonzero().flatten().tolist()}"
          f", of g_logits {torch.isnan(got['g_logits']).any(1).nonzero().flatten().tolist()}, "
          f"loss {float(got['loss'])} alpha_loss {float(got['alpha_loss'])}")
    for o in oc.DSAC_OUTPUTS:
        assert oc.same_nans(got[o], r64[o]), o
    assert bool(torch.isnan(got["loss"])) and bool(torch.isnan(got["g_log_alpha"]))
    for o in oc.DSAC_ROW_OUTPUTS:
        assert torch.equal(_bits(got[o][keep]), _bits(clean[o][keep])), o
    assert bool(torch.isfinite(clean["g_logits"]).all()) and bool(torch.isfinite(clean["loss"]))
    check_case(name, got, floor, r32)
    assert same_bits(got, run_dsac(dev, case))


def _masked_dsac_policy(dev, nets):
    from tianshou_amd.policy import DiscreteSACPolicy
    opt = {n: dsac_common.make_optim("adam", m.parameters()) for n, m in nets.items()}
    log_alpha = torch.zeros(1, requires_grad=True, device=dev)
    alpha = (0.98 * float(np.log(6)), log_alpha, dsac_common.make_optim("adam", [log_alpha], 3e-3))
    return DiscreteSACPolicy(nets["actor"], opt["actor"], nets["critic1"], opt["critic1"],
                             nets["critic2"], opt["critic2"], tau=0.01, gamma=0.99,
                             alpha=alpha).to(dev)


class _MaskedActor(lc.MaskedActor):
    """lc.MaskedActor with the legality table as a plain attribute: a module buffer keeps a
    DDPG-family update out of graph replay (DDPGPolicy._flat_ready)."""

    def __init__(self, dev):
        super().__init__(dev)
        illegal = self.illegal.to(dev)
        del self.illegal
        self.illegal = illegal


def test_learn_masked_actor_matches_torch_formulation(dev):
    """A DiscreteSACPolicy whose actor adds log(mask) to its logits (-inf over illegal actions;
    masked_fill's backward would hide a NaN gradient): three update() calls on the fused path
    (the first eager, the others replayed) and with fused = False, from the same weights, buffer
    and seed.  Every parameter stays finite on both legs and they agree at test_gpu_dsac.py's
    bound for its Adam variants (rtol 1e-5, atol 1e-6)."""
    from tianshou_amd.utils.net import DiscreteCritic, Net
    torch.manual_seed(41)
    nets = dict(actor=_MaskedActor(dev).to(dev))
    for k in ("critic1", "critic2"):
        nets[k] = DiscreteCritic(Net(8, hidden_sizes=(64, 64), device=dev), last_size=6,
                                 device=dev).to(dev)
    policy, twin = _masked_dsac_policy(dev, nets), _masked_dsac_policy(dev, copy.deepcopy(nets))
    twin.fused = False
    runs = []
    for pol in (policy, twin):
        pol.train()
        buf = lc.filled_buffer(dev, 8, 40, 8, lambda rng, E: rng.randint(0, 6, E), seed=42)
        with torch.no_grad():
            x = pol.actor(buf._meta.obs[:40])[0]
        assert bool(torch.isinf(x).any()) and bool(torch.isfinite(x).any(1).all())
        torch_leg = lc.count_calls(pol, "_learn_torch")
        np.random.seed(43)
        res = [pol.update(64, buf) for _ in range(3)]
        assert len(torch_leg) == (0 if pol is policy else 3)
        runs.append((res, dsac_common.flat_params(pol), float(pol._log_alpha.detach())))
    (res, par, la), (res_t, par_t, la_t) = runs
    for leg, r in (("fused", res), ("torch", res_t)):
        print(f"masked DiscreteSAC {leg}: actor losses", [u["loss/actor"] for u in r], "alpha",
              [u["alpha"] for u in r])
    print(f"masked DiscreteSAC: {int((~np.isfinite(par)).sum())} non-finite of {par.size} "
          f"parameters (torch leg {int((~np.isfinite(par_t)).sum())}), max |param - twin| "
          f"{np.abs(par - par_t).max():.3g}, log_alpha {la:.8g} / {la_t:.8g}, "
          f"{len(policy._learn_graphs)} learn graph")
    assert policy._flats and len(policy._learn_graphs) == 1 and not twin._learn_graphs
    assert np.isfinite(par).all() and np.isfinite(par_t).all(), "non-finite parameter"
    assert all(np.isfinite(list(u.values())).all() for u in res + res_t)
    np.testing.assert_allclose(par, par_t, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(la, la_t, rtol=1e-5, atol=1e-6)


# -- C51 and QR: wide rows -------------------------------------------------------------------------
def _wide(kind):
    return [n for n in oc.names(kind + "-b") if oc.CASES[n]["kind"] == kind]


@pytest.mark.parametrize("name", _wide("c51") + _wide("qr"))
def test_dist_loss_wide_rows(dev, floor, r32, name):
    """N = 255, 256, 257, 513 and 4096 (and QR's N = 1): a thread owns up to 16 atoms, the zero
    fill strides, the workgroup sum runs over four waves.  test_c51_loss_matches_f64's /
    test_qr_loss_matches_f64's other checks: zeros off the taken action, the same bits from a
    second launch, and for C51 an implied projected target that sums to 1."""
    case = oc.CASES[name]
    got = run_dist(dev, case)
    check_case(name, got, floor, r32)
    b, act = case["b"], case["act"].to(dev)
    rows = torch.arange(b, device=dev)
    grad = got["grad"]
    off = torch.ones_like(grad, dtype=torch.bool)
    off[rows, act] = False
    assert (grad[off] == 0).all()
    assert same_bits(got, run_dist(dev, case))
    if case["kind"] == "c51":
        w = torch.ones(b) if case["weight"] is None else case["weight"]
        scale = (case["curr"][torch.arange(b), case["act"]].double() + 1e-8) * b \
            / w.double().unsqueeze(1)
        implied = (-grad[rows, act].double().cpu() * scale).sum(1)
        want = (-oc.ref64(name)["grad"][torch.arange(b), case["act"]] * scale).sum(1)
        # test_c51_loss_matches_f64 holds this sum to 1 +- 1e-5.  A return between two atoms
        # gives them 1 - d / delta_z and 1 - d' / delta_z with d + d' the f32 atoms' distance,
        # which is delta_z to 2 ulp of v_max only: at N = 4096 (delta_z = 4.9e-3) the exact
        # projection sums to 1 within 3.9e-4 (the f64 reference: 1 + 1.25e-5).  So the kernel's
        # sum is held to the f64 reference's, at 1e-6: the gradient's N positive f32 entries
        # carry 2^-24 of their sum, 6e-8; and the reference's sum to 1 within that rounding.
        slack = 2 * float(_ulp(torch.tensor(oc.V_MAX))) / oc.delta_z(case["N"])
        print(f"{name}: implied target sums to 1 + {float((implied - 1).abs().max()):.2e} "
              f"(f64 {float((want - 1).abs().max()):.2e}, support rounding allows {slack:.2e})")
        assert float((want - 1).abs().max()) <= slack
        torch.testing.assert_close(implied, want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", [f"{k}-{w}" for k in ("c51", "qr") for w in oc.DIST_POISONS[k]])
def test_dist_loss_non_finite_inputs(dev, floor, r32, name):
    """NaN returns at an index below 256 and one above it, +-inf returns, a NaN and zeros in
    next: every output NaN (infinite) exactly where the f64 reference is, and the rows the
    poison does not touch bit for bit the clean run's."""
    case = oc.CASES[name]
    got, clean = run_dist(dev, case), run_case(dev, case["kind"] + "-clean")
    r64 = oc.ref64(name)
    r = oc.DIST_POISON_ROW
    act_r = int(case["act"][r])
    print(f"{name}: loss {float(got['loss'])} (f64 {float(r64['loss'])}), row {r}: vec "
          f"{float(got['vec'][r])} (f64 {float(r64['vec'][r])}), "
          f"{int(torch.isnan(got['grad'][r, act_r]).sum())} NaN of {case['N']} gradient entries "
          f"(f64 {int(torch.isnan(r64['grad'][r, act_r]).sum())})")
    for o in oc.DIST_OUTPUTS:
        assert oc.same_nans(got[o], r64[o]), o
        assert torch.equal(torch.isinf(got[o]).cpu(), torch.isinf(r64[o])), o
    keep = torch.ones(case["b"], dtype=torch.bool, device=dev)
    keep[r] = False
    for o in ("vec", "grad"):
        assert torch.equal(_bits(got[o][keep]), _bits(clean[o][keep])), o
    assert all(bool(torch.isfinite(clean[o]).all()) for o in oc.DIST_OUTPUTS)
    check_case(name, got, floor, r32)
    assert same_bits(got, run_dist(dev, case))


def test_dist_loss_width_limits_are_refused(dev):
    """N = 4097 (both losses) and C51's N = 1: the argument error, and none of the outputs
    written (they keep the sentinel they were prefilled with)."""
    L, s, p = _C.lib(), _C.stream_ptr(dev), _C.ptr
    b, A = 2, 1
    for fn, N in (("tsrl_c51_loss_fwd_bwd", _C.DIST_MAX_N + 1), ("tsrl_c51_loss_fwd_bwd", 1),
                  ("tsrl_qr_loss_fwd_bwd", _C.DIST_MAX_N + 1)):
        curr = torch.full((b, A, N), 1.0 / N, device=dev)
        rows = torch.full((b, N), 1.0 / N, device=dev)
        vec_n = torch.linspace(0.0, 1.0, N, device=dev)
        act = torch.zeros(b, dtype=torch.int64, device=dev)
        grad, vec, loss = (torch.full(sh, SENT, device=dev) for sh in ((b, A, N), (b,), ()))
        part = torch.full((b,), SENT, dtype=torch.float64, device=dev)
        if fn == "tsrl_c51_loss_fwd_bwd":
            rc = L.tsrl_c51_loss_fwd_bwd(p(curr), p(act), p(rows), p(rows), p(vec_n), None, b, A,
                                         N, 0.0, 1.0, 1.0 / max(N - 1, 1), p(grad), p(vec),
                                         p(part), p(loss), s)
        else:
            rc = L.tsrl_qr_loss_fwd_bwd(p(curr), p(act), p(rows), p(vec_n), None, b, A, N,
                                        p(grad), p(vec), p(part), p(loss), s)
        torch.cuda.synchronize()
        assert rc != 0, (fn, N)
        with pytest.raises(_C.TsrlError, match=fn):
            _C.check(rc, fn)
        for t in (grad, vec, loss, part):
            assert bool((t == SENT).all()), (fn, N)  # exactly the sentinel: nothing was written


# -- tsrl_dist_select past one workgroup trip and past the loss kernels' limit ---------------------
@pytest.mark.parametrize("name", list(oc.SELECT_CASES))
def test_dist_select_wide_rows(dev, name):
    """test_dist_select_matches_f64's checks at N = 1 and 255 .. 5000, on cases with clear gaps
    (tests/test_offpolicy_edges_host.py): q within 2 ulp of the f64 value rounded to f32, the
    action the f64 argmax on every row, the row an exact copy."""
    b, A, N, mode = oc.SELECT_CASES[name]
    sel, ev, w = oc.select_case(b, A, N, mode)
    q64 = oc.q_f64(sel, w)
    act_ref = q64.argmax(1).to(dev)
    sel, ev = sel.to(dev), ev.to(dev)
    w = None if w is None else w.to(dev)
    q, act, row = dist_select(sel, ev, w, want_q=True, want_row=True)
    ref32 = q64.float().to(dev)
    worst = ((q - ref32).abs() / _ulp(ref32)).max().item()
    print(f"{name}: q max {worst:.2f} ulp")
    assert worst <= 2.0
    assert act.dtype == torch.int64 and torch.equal(act, act_ref)
    rows = torch.arange(b, device=dev)
    assert torch.equal(row, ev[rows, act])
    assert torch.equal(dist_select(sel, None, w, want_row=True)[2], sel[rows, act])


# -- policies wider than the loss kernels ----------------------------------------------------------
@pytest.mark.parametrize("n", (_C.DIST_MAX_N, _C.DIST_MAX_N + 1))
@pytest.mark.parametrize("kind", ("c51", "qr", "rainbow"))
def test_wide_policy_update(dev, kind, n):
    """num_atoms / num_quantiles at the kernels' limit: update() runs the fused loss; one
    above it: learn() takes the torch formulation (no TsrlError from inside the update) while
    acting and the target selection stay on tsrl_dist_select.  The loss is finite."""
    from tianshou_amd.policy import C51Policy, QRDQNPolicy, RainbowPolicy
    from tianshou_amd.utils.net import Net, NoisyLinear
    torch.manual_seed(51)
    kw = {}
    if kind == "rainbow":
        head = {"hidden_sizes": (16,), "linear_layer": lambda x, y: NoisyLinear(x, y, 0.5)}
        kw["dueling_param"] = (dict(head), dict(head))
    net = Net(8, 2, hidden_sizes=(16,), device=dev, softmax=kind != "qr", num_atoms=n,
              **kw).to(dev)
    optim = torch.optim.Adam(net.parameters(), lr=1e-4)
    if kind == "qr":
        policy = QRDQNPolicy(net, optim, num_quantiles=n, target_update_freq=2).to(dev)
    else:
        cls = C51Policy if kind == "c51" else RainbowPolicy
        policy = cls(net, optim, num_atoms=n, target_update_freq=2).to(dev)
    policy.train()
    buf = lc.filled_buffer(dev, 4, 10, 8, lambda rng, E: rng.randint(0, 2, E), seed=52)
    torch_leg, fused_leg = lc.count_calls(policy, "_learn_torch"), \
        lc.count_calls(policy, "_fused_loss")
    np.random.seed(53)
    before = [p.detach().clone() for p in net.parameters()]
    res = policy.update(4, buf)
    print(f"{kind} N {n}: loss {res['loss']:.6g}, torch leg {len(torch_leg)}, fused "
          f"{len(fused_leg)}")
    assert np.isfinite(res["loss"])
    fused = n <= _C.DIST_MAX_N
    assert (len(torch_leg), len(fused_leg)) == ((0, 1) if fused else (1, 0))
    assert (policy._flat is not None) == fused
    assert any(not torch.equal(a, c) for a, c in zip(before, net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
