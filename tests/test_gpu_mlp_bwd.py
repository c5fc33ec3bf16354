"""The backward half of the fused actor/critic minibatch, kernel by kernel through the C ABI
(include/tsrl.h, csrc/mlp.hip), against float64 references built from the same f32 inputs.

* tsrl_mlp_dw (dw_x6_kernel + dw_reduce_kernel) against dZ1^T X[idx] in f64, elementwise and
  scaled by the absolute-product sum, at the row counts where the row split, the 32-row chunks
  and the masked / unmasked staging change, and at the widths where the db1 ones column sits
  on a 128-column tile edge.
* tsrl_ppo_tail_stage (ppo_tail16_kernel + tail_reduce_kernel) against f64 autograd that
  starts from the very H1 the kernel reads: dZ1, the layer-2/3 gradients, the loss sums and
  the finalised loss terms, per tensor as a scaled maximum.
* The fragment buffer's pad rows: both layer-1 kernels write them finite, the tail needs them
  finite and gives them no weight.

Bounds: the error of the kernel against f64 may be 4 x the error of torch's own f32 GPU
arithmetic on the same inputs against the same f64 reference (the margin of
test_fused_minibatch_matches_autograd), or a floor taken from the largest torch-f32 error over
the case list.  Every input lives in a table whose unreferenced rows and pad columns are NaN,
every workspace and output starts as NaN, and every output ends in a canary.
"""
import functools

import numpy as np
import pytest
import torch

from tests.mlp_common import frag_to_rows, gauss_dist, ppo_loss

pytestmark = pytest.mark.gpu

NAN = float("nan")
CANARY = -12345.0
NCAN = 64


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _out(numel, dev, dtype=torch.float32, ncan=NCAN):
    """An output of numel elements pre-filled with NaN, followed by ncan canary elements."""
    t = torch.full((numel + ncan,), NAN, dtype=dtype, device=dev)
    t[numel:] = CANARY
    return t


def _canary_ok(t, numel):
    return bool((t[numel:] == CANARY).all())


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _last_error():
    from tianshou_amd import _C
    return _C.lib().tsrl_last_error().decode(errors="replace")


# =============================================================================================
# 1. tsrl_mlp_dw
# =============================================================================================
# DW_FLOOR: per output group, the largest e of torch f32 (dz.T @ X[idx, :D] and dz.sum(0) on
# the GPU) over DW_CASES, rounded up to two digits; e = max_ij |got - G| / S with S =
# |dZ1|^T |X[idx]|.  It covers the cases where torch's own error is 0 or tiny (n = 1: a single
# rounding per element).  Next to each: the largest e of the kernel (bf16x6) and of torch f32
# over DW_CASES, measured on an MI355X.
DW_FLOOR = {
    "dW1": 4e-07,  # kernel 3.561e-07, torch f32 3.975e-07
    "db1": 7.9e-08,  # kernel 8.521e-08, torch f32 7.829e-08
}

# Row counts (dw_nsplit = max(1, min(170, n / 64)) rounded down to a multiple of 8 from 8 on;
# rps = the rows per split rounded up to whole 32-row chunks; dw_nsplit and tsrl_mlp_dw in
# csrc/mlp.hip):
#   1, 31, 32, 33   one split of one chunk (partial, partial, whole) / two chunks (whole + 1 row)
#   63, 64, 65      one split of two chunks (partial last, whole) / three (whole, whole, 1 row)
#   512             8 splits of exactly two whole chunks (the unmasked load and store)
#   520             rps 96: splits 0-4 whole, split 5 = 40 rows (whole + 8), splits 6, 7 empty
#   545             rps 96: split 5 = 65 rows (whole, whole, one row), splits 6, 7 empty
#   10881           n / 64 = 170 -> 168 splits, rps 96: 114 used, 54 trailing empty splits
DW_NS = (1, 31, 32, 33, 63, 64, 65, 512, 520, 545, 10881)
DW_WIDTHS = ((4, 4), (8, 8), (17, 20), (127, 128), (128, 128), (376, 376), (376, 384),
             (383, 384), (384, 384))
_MODES = ("none", "perm", "rep")


def _dw_cases():
    cases = []
    for i, n in enumerate(DW_NS):       # every n at D = 8 and D = 376, the idx mode cycling
        cases.append((n, 8, 8, _MODES[i % 3], "std"))
        cases.append((n, 376, 376, _MODES[(i + 1) % 3], "std"))
    for i, (D, ldx) in enumerate(DW_WIDTHS):   # every width at n = 33 and n = 545
        for n, mode in ((33, _MODES[(i + 2) % 3]), (545, _MODES[i % 3])):
            c = (n, D, ldx, mode, "std")
            if (n, D, ldx) not in [x[:3] for x in cases]:
                cases.append(c)
    for mode in _MODES:                 # the padded pitch under all three index modes
        for n in (520, 545):
            c = (n, 376, 384, mode, "std")
            if c not in cases:
                cases.append(c)
    # un-normalised observations (50 + 1e3 N(0,1)) against 1e-6-sized dZ1; exact zeros + denormals
    cases += [(545, 376, 384, "perm", "raw"), (33, 17, 20, "none", "raw"),
              (545, 376, 384, "rep", "zeros"), (65, 127, 128, "none", "zeros"),
              (10881, 383, 384, "perm", "zeros")]
    return cases


DW_CASES = _dw_cases()


def _dw_inputs(n, D, ldx, mode, kind):
    """(dz [n,128], table [N,ldx], idx or None) on the CPU; unreferenced table rows and the
    columns D..ldx of every row are NaN."""
    g = torch.Generator().manual_seed(1000003 * n + 1009 * D + 7 * ldx + _MODES.index(mode))
    if mode == "none":
        N, idx = n, None
    elif mode == "perm":
        N = n + 37
        idx = torch.randperm(N, generator=g)[:n]
    else:
        N = n // 2 + 5
        idx = torch.randint(0, N, (n,), generator=g)
    rows = torch.arange(N) if idx is None else idx
    if kind == "raw":
        x = 50.0 + 1e3 * torch.randn(N, D, generator=g)
        dz = 1e-6 * torch.randn(n, 128, generator=g)
    else:
        x = torch.randn(N, D, generator=g)
        dz = 1e-3 * torch.randn(n, 128, generator=g)
    if kind == "zeros":
        x[:, 1:min(D, 4)] = 0.0            # whole columns: S == 0, the result exactly 0
        x[: N // 2, D // 2:] = 0.0         # a block
        dz[:, 7] = 0.0                     # a whole feature (actor), and one of the critic's
        dz[:, 64 + 31] = 0.0
        dz[n // 3:, 40:50] = 0.0
        sub = torch.tensor([1e-40, -3e-41, 1.4e-45, -1e-39])
        for j in range(min(n, 4)):         # a few denormals among normal values
            x[rows[j], 0] = sub[j]
            dz[j, (11 * j + 3) % 128] = sub[3 - j]
    X = torch.full((N, ldx), NAN)
    X[:, :D] = x
    if idx is not None:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        X[dead] = NAN
    return dz, X, idx


def _dw_scaled_err(gW, gb, G, gB, S, Sb, exact_zero):
    """max |got - ref| / S over dW1 and db1; where S == 0 the result must be exactly 0
    (asserted for the kernel, exact_zero)."""
    out = []
    for got, ref, s in ((gW, G, S), (gb, gB, Sb)):
        z = s == 0
        if exact_zero:
            assert bool((got[z] == 0).all()), "non-zero result where every product is zero"
        nz = ~z
        out.append(float(((got - ref).abs()[nz] / s[nz]).max()) if bool(nz.any()) else 0.0)
    return out


@pytest.mark.parametrize("n,D,ldx,mode,kind", DW_CASES)
def test_dw_matches_f64(dev, n, D, ldx, mode, kind):
    """tsrl_mlp_dw against G = dZ1^T X[idx, :D] and gb = column sums of dZ1 in f64, split at
    feature 64 into the actor's and the critic's halves: e = max |got - G| / (|dZ1|^T |X|)
    within max(4 x torch f32's e, DW_FLOOR); exactly 0 where every product is 0.  NaN in every
    table row idx does not name, in the columns D..ldx, in the partials workspace and in the
    four outputs; canaries behind the outputs; a second call into the same buffers gives the
    same bits (overwrite, not accumulate).  Row counts as DW_NS above."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    dz, X, idx = _dw_inputs(n, D, ldx, mode, kind)
    xi = (X if idx is None else X[idx])[:, :D]
    assert bool(torch.isfinite(xi).all())
    G = dz.double().T @ xi.double()
    gB = dz.double().sum(0)
    S = dz.abs().double().T @ xi.abs().double()
    Sb = dz.abs().double().sum(0)
    dz_d, X_d = dz.to(dev), X.to(dev)
    idx_d = None if idx is None else idx.to(dev)
    wsb = int(L.tsrl_mlp_dw_workspace_bytes(n, D))
    assert wsb % 4 == 0
    ws = torch.full((wsb // 4,), NAN, device=dev)
    gWa, gWc = _out(64 * D, dev), _out(64 * D, dev)
    gba, gbc = _out(64, dev), _out(64, dev)

    def call():
        _C.check(L.tsrl_mlp_dw(_C.ptr(dz_d), _C.ptr(X_d), ldx, _C.ptr(idx_d), n, D, _C.ptr(gWa),
                               _C.ptr(gba), _C.ptr(gWc), _C.ptr(gbc), _C.ptr(ws), wsb, s),
                 "tsrl_mlp_dw")
        torch.cuda.synchronize()
        return [t.clone() for t in (gWa, gba, gWc, gbc)]

    first = call()
    second = call()
    for a, b in zip(first, second):
        assert torch.equal(_bits(a), _bits(b)), "second call differs: accumulate or race"
    for t, m in ((gWa, 64 * D), (gWc, 64 * D), (gba, 64), (gbc, 64)):
        assert _canary_ok(t, m)
        assert bool(torch.isfinite(t[:m]).all())
    gW = torch.cat([gWa[:64 * D].view(64, D), gWc[:64 * D].view(64, D)]).cpu().double()
    gb = torch.cat([gba[:64], gbc[:64]]).cpu().double()
    xg = (X_d if idx_d is None else X_d[idx_d])[:, :D]
    tW = (dz_d.T @ xg).cpu().double()
    tb = dz_d.sum(0).cpu().double()
    ek = _dw_scaled_err(gW, gb, G, gB, S, Sb, True)
    et = _dw_scaled_err(tW, tb, G, gB, S, Sb, False)
    print(f"BWD dw n={n} D={D} ldx={ldx} {mode} {kind}: dW1 e_kernel {ek[0]:.4g} e_torch_f32 "
          f"{et[0]:.4g}; db1 e_kernel {ek[1]:.4g} e_torch_f32 {et[1]:.4g}")
    for what, k, t in (("dW1", ek[0], et[0]), ("db1", ek[1], et[1])):
        if k > max(4 * t, DW_FLOOR[what]):
            err = (gW - G).abs() / S.clamp_min(1e-300)
            f, c = divmod(int(err.argmax()), D)
            pytest.fail(f"{what}: e_kernel {k:.3g} > max(4 x {t:.3g}, {DW_FLOOR[what]:.3g}); worst "
                        f"dW1 element feature {f} (tile {f // 32}), column {c} (tile "
                        f"{c // 128})")


def test_dw_argument_errors(dev):
    """A workspace one byte short, a pitch below roundup(D, 4), a pitch that is no multiple of
    4 and n == 0 are argument errors that name the entry point; nothing is launched."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    n, D = 33, 17
    dz = torch.zeros(n, 128, device=dev)
    X = torch.zeros(n, 24, device=dev)
    wsb = int(L.tsrl_mlp_dw_workspace_bytes(n, D))
    ws = torch.full((wsb // 4,), NAN, device=dev)
    outs = [_out(64 * D, dev), _out(64, dev), _out(64 * D, dev), _out(64, dev)]

    def call(n_, ldx, wsb_):
        return L.tsrl_mlp_dw(_C.ptr(dz), _C.ptr(X), ldx, None, n_, D, _C.ptr(outs[0]),
                             _C.ptr(outs[1]), _C.ptr(outs[2]), _C.ptr(outs[3]), _C.ptr(ws),
                             wsb_, s)

    for what, args in (("ws one short", (n, 20, wsb - 1)), ("ldx < roundup(D, 4)", (n, 16, wsb)),
                       ("ldx % 4", (n, 18, wsb)), ("n == 0", (0, 20, wsb))):
        assert call(*args) != 0, what
        assert "tsrl_mlp_dw" in _last_error(), (what, _last_error())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws).all())
    for t, m in zip(outs, (64 * D, 64, 64 * D, 64)):
        assert bool(torch.isnan(t[:m]).all()) and _canary_ok(t, m)
    assert call(n, 20, wsb) == 0   # the same buffers with good arguments
    torch.cuda.synchronize()


# =============================================================================================
# 2. tsrl_ppo_tail_stage
# =============================================================================================
# TAIL_FLOOR: per output tensor, the project's floor for this path (2e-6, on relative L2, in
# test_fused_minibatch_matches_autograd), raised where torch f32 itself -- the same graph in f32
# on the GPU -- is further from f64 somewhere in TAIL_CASES + PAD_CASES: then its largest e there,
# rounded up to two digits; e = max |got - ref| / max |ref|.  Next to each: the largest e of the
# kernel and of torch f32 over those cases, measured on an MI355X.  The actor's tensors carry
# the f32 spacing of log pi (about -1.4 A: 1.9e-6 at A = 17, 3.8e-6 at A = 32) through the
# ratio exp(logp - logp_old); b3c is one element, a sum of per-row terms that cancel.
TAIL_FLOOR = {
    "dz1": 4.8e-06,  # kernel 5.986e-06, torch f32 4.721e-06
    "w2a": 4.4e-06,  # kernel 3.189e-06, torch f32 4.361e-06
    "b2a": 4.4e-06,  # kernel 3.893e-06, torch f32 4.39e-06
    "w2c": 2.6e-06,  # kernel 4.672e-07, torch f32 2.589e-06
    "b2c": 2e-06,  # kernel 6.384e-07, torch f32 6.613e-07
    "w3a": 3.7e-06,  # kernel 4.648e-06, torch f32 3.606e-06
    "b3a": 3.4e-06,  # kernel 5.936e-06, torch f32 3.329e-06
    "w3c": 2e-06,  # kernel 4.265e-07, torch f32 5.481e-07
    "b3c": 0.00037,  # kernel 0.0001903, torch f32 0.0003666
    "grad_log_std": 3.2e-06,  # kernel 5.817e-06, torch f32 3.192e-06
    "dlogstd": 3.9e-06,  # kernel 3.47e-05, torch f32 3.849e-06
}

# d/dlog_std[a] = sum over the rows of g_i (d_ia^2 / sigma_a^2 - 1), g_i = dL/dlogp_i: terms of
# both signs that cancel (normalised advantages sum to zero) down to about 1 / sqrt(n) of
# sum |term|, while 1 / sigma_a^2 is ONE f32 constant per action whose rounding does not
# average out over the rows: from log sigma through expf (1 ulp = 2^-23 relative), a square
# (twice that + 1/2) and a reciprocal (+ 1/2) it may be 3.5 ulp off, 4 with the per-row
# roundings, and moves the sum by that relative error times sum_i g_i d_ia^2 / sigma_a^2.
# max |ref| does not see the uncancelled size, so for the two log-std outputs the bound is
# also at least LS_ULPS ulps of max_a sum_i |term_ia| (from the f64 reference) over max |ref|.
# The one case that needs it, measured (n = 1000, A = 1, defaults, where torch's constant
# happens to round well): kernel e 3.47e-5 on the sums' entry (error 5.8e-8 absolute, |ref|
# 1.7e-3) and 5.82e-6 on grad_log_std, torch f32 3.85e-6 and 6.5e-8; every other case is
# within 4 x torch f32 or the floors above.
LS_ULPS = 4

H = 64
TAIL_D = 8
TAIL_NS = (1, 15, 16, 17, 31, 33, 127, 128, 129, 1000, 32789)
TAIL_AS = (1, 6, 16, 17, 32)
TAIL_SETS = {
    "default": {},
    "dual_vclip": dict(dual_clip=3.0, value_clip=True),
    "raw_adv": dict(norm_adv=False, ent_coef=0.0),
    "a2c": dict(a2c=True),
}
GRADS = ("w2a", "b2a", "w2c", "b2c", "w3a", "b3a", "w3c", "b3c")


def _tail_cases():
    cases = []
    for i, n in enumerate(TAIL_NS):       # every n at A = 6 and A = 17 on the defaults
        cases.append((n, 6, "default", bool(i & 1)))
        cases.append((n, 17, "default", not (i & 1)))
    cases.append((1, 6, "raw_adv", True))  # n = 1 with a defined reference (see _tail_ref)
    cases.append((1, 17, "raw_adv", False))
    for i, A in enumerate(TAIL_AS):       # every A and every parameter set at n = 33 and 1000
        for j, ps in enumerate(TAIL_SETS):
            for n in (33, 1000):
                c = (n, A, ps, bool((i + j + (n > 33)) & 1))
                if c[:3] not in [x[:3] for x in cases]:
                    cases.append(c)
    return cases


TAIL_CASES = _tail_cases()


def _a2c():
    from tests import test_gpu_a2c
    return test_gpu_a2c


def _tail_params(n, kw):
    from tianshou_amd import _C
    if kw.get("a2c"):
        return _a2c()._params(n)
    p = _C.PPOParams()
    p.eps_clip, p.dual_clip = 0.2, kw.get("dual_clip") or 0.0
    p.vf_coef, p.ent_coef, p.adv_eps = 0.25, kw.get("ent_coef", 0.01), 1e-8
    p.b_global = float(n)
    p.value_clip, p.norm_adv = int(bool(kw.get("value_clip"))), int(kw.get("norm_adv", True))
    return p


def _l1_frag(dev, l1, X, ldx, idx, n, D, Wa, ba, Wc, bc, frag_out=1, prefill=NAN):
    """Layer 1 (tanh) of n rows through tsrl_mlp_l1_fwd ("f32") or tsrl_mlp_split_w +
    tsrl_mlp_l1_fwd_x6 ("x6") into a pre-filled buffer: fragment layout or row-major."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    numel = int(L.tsrl_mlp_frag_floats(n)) if frag_out else n * 128
    out = torch.full((numel + NCAN,), prefill, device=dev)
    out[numel:] = CANARY
    if l1 == "x6":
        ws = torch.full(((int(L.tsrl_mlp_split_bytes(D)) + 3) // 4,), NAN, device=dev)
        _C.check(L.tsrl_mlp_split_w(_C.ptr(Wa), _C.ptr(Wc), D, _C.ptr(ws), s))
        _C.check(L.tsrl_mlp_l1_fwd_x6(_C.ptr(X), ldx, _C.ptr(idx), n, D, _C.ptr(ws), _C.ptr(ba),
                                      _C.ptr(bc), 1, _C.ptr(out), frag_out, s))
    else:
        _C.check(L.tsrl_mlp_l1_fwd(_C.ptr(X), ldx, _C.ptr(idx), n, D, _C.ptr(Wa), _C.ptr(ba),
                                   _C.ptr(Wc), _C.ptr(bc), 1, _C.ptr(out), frag_out, s))
    torch.cuda.synchronize()
    assert _canary_ok(out, numel)
    return out[:numel]


def _tail_ref(H1, W, mb, kw, n, dtype, device):
    """Layers 2-3 of both nets on the given H1, the PPO (mlp_common.ppo_loss) or A2C
    (test_gpu_a2c._a2c_loss) loss and its autograd: every output of tsrl_ppo_tail_stage.

    n == 1 with norm_adv: torch's unbiased std of one value is NaN, so the formula has no
    reference there; the kernel takes that variance as 0 and the normalised advantage is
    (adv - adv) / (0 + 1e-8) = 0.  The reference states that value: adv = 0, no normalisation."""
    c = lambda t: None if t is None else t.to(device, dtype)  # noqa: E731
    P = {k: v.detach().to(device, dtype).clone().requires_grad_(True) for k, v in W.items()}
    h = H1.to(device, dtype).clone().requires_grad_(True)
    ha = torch.tanh(h[:, :H] @ P["w2a"].T + P["b2a"])
    mu = ha @ P["w3a"].T + P["b3a"]
    hc = torch.tanh(h[:, H:] @ P["w2c"].T + P["b2c"])
    value = (hc @ P["w3c"].T + P["b3c"]).flatten()
    # one copy of log sigma per row: its gradient is each row's share of d/dlog_std
    srows = P["sigma"].view(1, -1) + torch.zeros_like(mu)
    dist = gauss_dist(mu, srows)
    act, logp_old, adv, ret, v_s = (c(mb[k]) for k in ("act", "logp_old", "adv", "ret", "v_s"))
    if kw.get("a2c"):
        terms = _a2c()._a2c_loss(dist, value, act, adv, ret)
    else:
        kw = dict(kw)
        if n == 1 and kw.get("norm_adv", True):
            adv, kw["norm_adv"] = torch.zeros_like(adv), False
        terms = ppo_loss(dist, value, act, logp_old, adv, ret, v_s, kw)
    d = lambda t: t.detach().cpu().double()  # noqa: E731
    # sums [4 + A]: clip (or actor) sum, vf sum, row count, unused, d(policy term)/dlog_std
    out = {"dlogstd": d(torch.autograd.grad(terms[1], P["sigma"], retain_graph=True)[0]),
           "ls_abs": d(torch.autograd.grad(terms[1], srows, retain_graph=True)[0]).abs().sum(0)}
    terms[0].backward()
    out.update({k: d(P[k].grad) for k in GRADS})
    out["dz1"] = d(h.grad * (1.0 - h * h))
    out["grad_log_std"] = d(P["sigma"].grad)
    t = torch.stack([d(x) for x in terms])
    out["losses"] = t
    out["sum01"] = t[1:3] * n
    return out


@functools.lru_cache(maxsize=None)
def _tail_case(n, A, pset, use_idx, l1="x6"):
    """Inputs of one tail case on the device, the f64 CPU reference and torch's f32 GPU run of
    the same graph; computed once per case and shared (nothing in it is written afterwards)."""
    dev = torch.device("cuda", 0)
    kw = TAIL_SETS[pset]
    g = torch.Generator().manual_seed(7919 * n + 101 * A + list(TAIL_SETS).index(pset))
    D = TAIL_D
    N = n + 29 if use_idx else n
    idx = torch.randperm(N, generator=g)[:n] if use_idx else None
    X = torch.randn(N, D, generator=g)
    if use_idx:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        X[dead] = NAN
    r = lambda *s, k=1.0: (k * torch.randn(*s, generator=g))  # noqa: E731
    W1 = [t.to(dev) for t in (r(H, D, k=0.4), r(H, k=0.2), r(H, D, k=0.4), r(H, k=0.2))]
    W = {"w2a": r(H, H, k=0.15), "b2a": r(H, k=0.1), "w2c": r(H, H, k=0.15), "b2c": r(H, k=0.1),
         "w3a": r(A, H, k=0.15), "b3a": r(A, k=0.1), "w3c": r(1, H, k=0.15), "b3c": r(1, k=0.1),
         "sigma": r(A, k=0.3) - 0.5}
    idx_d = None if idx is None else idx.to(dev)
    frag = _l1_frag(dev, l1, X.to(dev), D, idx_d, n, D, W1[0], W1[1], W1[2], W1[3])
    H1 = frag_to_rows(frag, n)
    assert bool(torch.isfinite(H1).all())
    # actions as a rollout stores them, mu + sigma eps (log pi about -1.4 A; actions drawn
    # without regard to mu put it near -2.7 A, and at A = 32, n = 33 the f32 spacing of that
    # alone -- torch f32 included -- moves the clip term by more than the atol of 1e-6)
    with torch.no_grad():
        mu = torch.tanh(H1[:, :H] @ W["w2a"].T + W["b2a"]) @ W["w3a"].T + W["b3a"]
        mb = {"act": mu + W["sigma"].exp() * r(n, A), "adv": r(n, k=2.0) + 0.3, "ret": r(n)}
        mb["v_s"] = mb["ret"] + r(n, k=0.3)
        mb["logp_old"] = gauss_dist(mu, W["sigma"]).log_prob(mb["act"]) + r(n, k=0.2)
    tab = {}
    for k, v in mb.items():       # tables in buffer order: unreferenced rows NaN
        if idx is None:
            tab[k] = v.to(dev)
        else:
            t = torch.full((N,) + tuple(v.shape[1:]), NAN)
            t[idx] = v
            tab[k] = t.to(dev)
    adv64 = mb["adv"].double()
    adv_sums = torch.stack([adv64.sum(), (adv64 * adv64).sum()]).to(dev)
    ref = _tail_ref(H1, W, mb, kw, n, torch.float64, "cpu")
    t32 = _tail_ref(H1, W, mb, kw, n, torch.float32, dev)
    return dict(n=n, A=A, kw=kw, idx=idx_d, frag=frag, W={k: v.to(dev) for k, v in W.items()},
                tab=tab, adv_sums=adv_sums, ref=ref, t32=t32)


# output name -> (numel, dtype, canary length); the kernel pads the actions to 32 internally, so
# the canaries of the actor head's gradients span that padding
def _tail_outputs(n, A, dev):
    spec = {"dz1": (n * 128, torch.float32, NCAN),
            "w2a": (H * H, torch.float32, NCAN), "b2a": (H, torch.float32, NCAN),
            "w2c": (H * H, torch.float32, NCAN), "b2c": (H, torch.float32, NCAN),
            "w3a": (A * H, torch.float32, max(NCAN, (32 - A) * H + NCAN)),
            "b3a": (A, torch.float32, NCAN), "w3c": (H, torch.float32, NCAN),
            "b3c": (1, torch.float32, NCAN), "sums": (4 + A, torch.float64, NCAN),
            "losses": (4, torch.float32, NCAN), "grad_log_std": (A, torch.float32, NCAN)}
    return spec, {k: _out(m, dev, dt, nc) for k, (m, dt, nc) in spec.items()}


def _run_tail(dev, case, stages=(3,), fin=True, fin_override=None):
    """tsrl_ppo_tail_stage on the case into fresh NaN-filled buffers (workspace included), one
    call per entry of stages on the current stream.  Returns {name: tensor without canary}."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    n, A, kw, W, tab = case["n"], case["A"], case["kw"], case["W"], case["tab"]
    spec, o = _tail_outputs(n, A, dev)
    wsb = int(L.tsrl_ppo_tail_workspace_bytes(n))
    ws = torch.full(((wsb + 3) // 4,), NAN, device=dev)
    tw = _C.TailWeights(*[_C.ptr(W[k]) for k in GRADS], _C.ptr(W["sigma"]))
    tg = _C.TailGrads(*[_C.ptr(o[k]) for k in GRADS])
    a2c = bool(kw.get("a2c"))
    p = _tail_params(n, kw)
    fin_ptrs = (_C.ptr(W["sigma"]), _C.ptr(o["losses"]), _C.ptr(o["grad_log_std"])) if fin \
        else (None, None, None)
    if fin_override is not None:
        fin_ptrs = tuple(q if keep else None for q, keep in zip(fin_ptrs, fin_override))
    rcs = []
    for st in stages:
        rcs.append(L.tsrl_ppo_tail_stage(
            _C.ptr(case["frag"]), n, _C.ptr(case["idx"]), tw, A, _C.ptr(tab["act"]),
            None if a2c else _C.ptr(tab["logp_old"]), _C.ptr(tab["adv"]), _C.ptr(tab["ret"]),
            None if a2c else _C.ptr(tab["v_s"]),
            _C.ptr(case["adv_sums"]) if p.norm_adv else None, p, _C.ptr(o["dz1"]), tg,
            _C.ptr(o["sums"]), _C.ptr(ws), wsb, *fin_ptrs, st, s))
    torch.cuda.synchronize()
    if fin_override is not None:
        return rcs, o, spec
    for rc in rcs:
        _C.check(rc, "tsrl_ppo_tail_stage")
    res = {}
    for k, (m, _, _) in spec.items():
        assert _canary_ok(o[k], m), f"{k}: written past its {m} elements"
        res[k] = o[k][:m]
    return res


def _tensor_err(got, ref):
    """max |got - ref| / max |ref|; a reference that is all zero asks for exact zeros."""
    den = float(ref.abs().max())
    if den == 0.0:
        return 0.0 if bool((got == 0).all()) else float("inf")
    return float((got - ref).abs().max()) / den


def _check_tail(case, res, tag):
    """Every output of one finalising tail run against the case's f64 reference, bounded by
    torch f32's error on the same graph; prints both per tensor."""
    n, A, ref, t32 = case["n"], case["A"], case["ref"], case["t32"]
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), f"{k} not finite"
    got = {k: res[k].cpu().double().view(ref[k].shape) for k in GRADS}
    got["dz1"] = res["dz1"].cpu().double().view(n, 128)
    got["grad_log_std"] = res["grad_log_std"].cpu().double().view(ref["grad_log_std"].shape)
    sums = res["sums"].cpu()
    got["dlogstd"] = sums[4:].view(ref["dlogstd"].shape)
    assert float(sums[2]) == float(n)
    bad = []
    for k in ("dz1",) + GRADS + ("grad_log_std", "dlogstd"):
        ek, et = _tensor_err(got[k], ref[k]), _tensor_err(t32[k], ref[k])
        print(f"BWD tail {tag} {k}: e_kernel {ek:.4g} e_torch_f32 {et:.4g}")
        bound = max(4 * et, TAIL_FLOOR[k])
        if k in ("grad_log_std", "dlogstd") and float(ref[k].abs().max()) > 0.0:
            bound = max(bound, LS_ULPS * 2.0 ** -23 * float(ref["ls_abs"].max())
                        / float(ref[k].abs().max()))
        if not ek <= bound:
            err = (got[k] - ref[k]).abs().flatten()
            bad.append((k, ek, et, int(err.argmax())))
    np.testing.assert_allclose(res["losses"].cpu().double().numpy(), ref["losses"].numpy(),
                               rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(sums[:2].numpy(), ref["sum01"].numpy(), rtol=1e-5, atol=1e-6 * n)
    assert not bad, f"(tensor, e_kernel, e_torch_f32, flat index of the worst element): {bad}"


@pytest.mark.parametrize("n,A,pset,use_idx", TAIL_CASES)
def test_tail_matches_f64_autograd(dev, n, A, pset, use_idx):
    """tsrl_ppo_tail_stage (stages = 3, finalising) on the fragment buffer tsrl_mlp_l1_fwd_x6
    wrote, against f64 autograd that starts from those exact H1 values: dZ1 = dL/dH1 (1 - H1^2),
    the eight layer-2/3 gradients, the log-std gradient, losses[4] and sums[4 + A] (count == n
    exactly).  Per tensor max |got - ref| / max |ref| within max(4 x torch f32's, TAIL_FLOOR),
    for the log-std outputs also LS_ULPS ulps of the uncancelled sum (see LS_ULPS).
    Rows 1..17, 31, 33 and 127..129 leave dead lanes in the 16-row tiles; 32789 is past 256
    workgroups x 8 waves x 16 rows, so some waves take a second tile and the last tile has 5
    live rows.  A = 16 fills the first 16-action tile, 17 spills into the second, 32 is the
    maximum.  With idx, the rows of act / logp_old / adv / ret / v_s that idx does not name
    are NaN; the A2C objective runs with logp_old, v_s and adv_sums NULL.  adv_sums comes from
    the host in f64."""
    case = _tail_case(n, A, pset, use_idx)
    res = _run_tail(dev, case)
    _check_tail(case, res, f"n={n} A={A} {pset} idx={int(use_idx)}")


@pytest.mark.parametrize("n", [17, 1000])
@pytest.mark.parametrize("A", [6, 17])
def test_tail_stages_bitwise(dev, n, A):
    """stages = 3 in one call, and 4, 8, 2 as three calls on the same stream into fresh
    NaN-filled buffers: every output bit for bit the same."""
    case = _tail_case(n, A, "default", bool(TAIL_NS.index(n) & 1) ^ (A == 17))
    one = _run_tail(dev, case, stages=(3,))
    three = _run_tail(dev, case, stages=(4, 8, 2))
    for k in one:
        assert bool(torch.isfinite(three[k]).all()), k
        assert torch.equal(_bits(one[k]), _bits(three[k])), k


def test_tail_without_finalisation(dev):
    """log_std / losses / grad_log_std all NULL: the same sums and gradients bit for bit as
    the finalising call, losses and grad_log_std untouched; only some of the three given is an
    argument error that names the entry point and launches nothing."""
    case = _tail_case(1000, 17, "default", False)
    fin = _run_tail(dev, case)
    raw = _run_tail(dev, case, fin=False)
    for k in fin:
        if k in ("losses", "grad_log_std"):
            assert bool(torch.isnan(raw[k]).all()), k
        else:
            assert torch.equal(_bits(fin[k]), _bits(raw[k])), k
    for keep in ((True, False, False), (False, True, False), (False, False, True),
                 (True, True, False)):
        rcs, o, spec = _run_tail(dev, case, fin_override=keep)
        assert rcs[0] != 0, keep
        assert "tsrl_ppo_tail_stage" in _last_error(), (keep, _last_error())
        for k, (m, _, _) in spec.items():
            assert bool(torch.isnan(o[k][:m]).all()) and _canary_ok(o[k], m), (keep, k)


# =============================================================================================
# 3. The fragment buffer's pad rows
# =============================================================================================
@pytest.mark.parametrize("l1", ["f32", "x6"])
@pytest.mark.parametrize("D", [8, 376])
@pytest.mark.parametrize("n,use_idx", [(1, False), (1, True), (33, False), (33, True),
                                       (129, False), (129, True), (257, False), (257, True),
                                       (1000, False), (1000, True)])
def test_l1_writes_every_fragment_float_finite(dev, l1, D, n, use_idx):
    """include/tsrl.h, the writing side: with frag_out = 1 (tanh) tsrl_mlp_l1_fwd and
    tsrl_mlp_l1_fwd_x6 overwrite all tsrl_mlp_frag_floats(n) floats of a NaN-filled buffer
    with finite values (and nothing behind them), pad rows included, and rows < n equal the
    row-major output bit for bit.  Table rows idx does not name are NaN.  n = 257 puts one
    live row into the second 256-row tile of the ring kernel."""
    g = torch.Generator().manual_seed(31 * n + D + use_idx)
    N = n + 50 if use_idx else n
    X = 2.0 * torch.randn(N, D, generator=g)
    idx = torch.randperm(N, generator=g)[:n] if use_idx else None
    if use_idx:
        dead = torch.ones(N, dtype=torch.bool)
        dead[idx] = False
        X[dead] = NAN
    Wa, Wc = (0.1 * torch.randn(H, D, generator=g)).to(dev), \
        (0.1 * torch.randn(H, D, generator=g)).to(dev)
    ba, bc = torch.randn(H, generator=g).to(dev), torch.randn(H, generator=g).to(dev)
    X_d, idx_d = X.to(dev), None if idx is None else idx.to(dev)
    frag = _l1_frag(dev, l1, X_d, D, idx_d, n, D, Wa, ba, Wc, bc, frag_out=1)
    rows = _l1_frag(dev, l1, X_d, D, idx_d, n, D, Wa, ba, Wc, bc, frag_out=0)
    assert bool(torch.isfinite(frag).all()), \
        f"{int((~torch.isfinite(frag)).sum())} of {frag.numel()} fragment floats not written"
    assert bool(torch.isfinite(rows).all())
    assert torch.equal(_bits(frag_to_rows(frag, n)), _bits(rows.view(n, 128).cpu()))


PAD_CASES = [(33, 6, True), (1000, 17, False)]


@pytest.mark.parametrize("n,A,use_idx", PAD_CASES)
def test_tail_gives_pad_rows_no_weight(dev, n, A, use_idx):
    """include/tsrl.h, the requiring side: the same tail case on the fragment buffer of each
    layer-1 kernel -- pad rows tanh(bias) from tsrl_mlp_l1_fwd, a copy of row n - 1 from
    tsrl_mlp_l1_fwd_x6 -- meets the bound of test_tail_matches_f64_autograd against the f64
    reference built from that buffer's own live rows; and with the pad rows of the x6 buffer
    overwritten by other finite values every output keeps its bits."""
    for l1 in ("f32", "x6"):
        case = _tail_case(n, A, "default", use_idx, l1)
        res = _run_tail(dev, case)
        _check_tail(case, res, f"n={n} A={A} l1={l1}")
    # rows n.. of the last 32-row fragment tile: lanes (row & 31) and (row & 31) + 32
    frag2 = case["frag"].clone()
    last = (n - 1) // 32
    tile = frag2[last * 4 * 1024:(last + 1) * 4 * 1024].view(4, 4, 64, 4)
    lanes = torch.arange(64, device=dev)
    pad = (lanes & 31) + 32 * last >= n
    assert bool(pad.any())
    tile[:, :, pad, :] = 0.625
    res2 = _run_tail(dev, dict(case, frag=frag2))
    for k in res:
        assert torch.equal(_bits(res[k]), _bits(res2[k])), k
