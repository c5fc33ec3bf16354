"""Cases and references shared by tests/test_gpu_offpolicy_edges.py (the off-policy loss
kernels of csrc/dsac.hip and csrc/dqn_dist.hip at masked (-inf) logits, extreme logits, NaN and
infinite inputs, and the widths at which a thread owns several atoms, up to the limit) and
tests/test_offpolicy_edges_host.py (which checks on the CPU that every case is what it claims).

One reference function per kernel family, in torch, evaluated at float64 (the reference) and at
float32 (the torch formulation):

``dsac_ref``   discrete_sac.py:93-97 (the soft state value) and :127-144 (the actor and
               temperature losses, their gradients by autograd) over loss_edges_common.cat_dist,
               which is torch's Categorical(logits=x) with the clamp of the normalised logit at
               float32's lowest value at either precision;
``dist_rows``  test_gpu_dist_dqn.py's c51_reference / qr_reference one batch row at a time
               (their [b, N, N] intermediates at N = 4096 are 134 MB per row in f64).
"""
import functools
import math

import torch

from tests import loss_edges_common as lc
from tests.test_gpu_dist_dqn import (V_MAX, V_MIN, c51_inputs, c51_reference, qr_inputs,
                                     qr_reference)
from tests.test_gpu_dist_dqn import q_f64, top2_rel_gap  # noqa: F401  (re-exported)
from tianshou_amd import _C

INF = lc.INF
NAN = float("nan")
scaled_err = lc.scaled_err


def _f32(v):
    """The float32 value nearest v, as a Python float: what the kernel reads from its f32
    temperature tensors."""
    return float(torch.tensor(v, dtype=torch.float32))


ALPHA, LOG_ALPHA = _f32(0.37), _f32(-0.8)

# -- DiscreteSAC --------------------------------------------------------------------------------
DSAC_OUTPUTS = ("target", "loss", "alpha_loss", "g_logits", "g_log_alpha")
DSAC_ROW_OUTPUTS = ("target", "g_logits")  # one row per batch row
DSAC_BS = (1, 5, 65)
DSAC_AS = (2, 6, 18, 65, 130)  # 130: three trips of a 64-lane group, the last of 2 columns


def dsac_ref(case, dtype, device="cpu"):
    """The five outputs of tsrl_dsac_target and tsrl_dsac_actor_loss_fwd_bwd at ``dtype``."""
    cast = lambda k: case[k].detach().to(device=device, dtype=dtype).clone()  # noqa: E731
    x = cast("logits").requires_grad_(True)
    q = torch.min(cast("q1"), cast("q2"))
    log_alpha = torch.tensor([LOG_ALPHA], dtype=dtype, device=device, requires_grad=True)
    _, probs, ent = lc.cat_dist(x, 0)
    v = (probs * q).sum(dim=-1)
    target = v + ALPHA * ent                                          # discrete_sac.py:93-97
    loss = -(ALPHA * ent + v).mean()                                  # :127-133
    alpha_loss = -(log_alpha * (-ent.detach() + case["te"])).mean()   # :138-140
    (g_logits,) = torch.autograd.grad(loss, x)
    (g_la,) = torch.autograd.grad(alpha_loss, log_alpha)
    out = dict(target=target, loss=loss, alpha_loss=alpha_loss, g_logits=g_logits,
               g_log_alpha=g_la.reshape(()))
    return {k: t.detach().cpu() for k, t in out.items()}


def _dsac_base(seed, b, A):
    """tests/test_gpu_dsac.py's inputs: logits of std 2, Q tables around 1, every third row of
    q2 tying q1."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, A, generator=g) * 2.0
    q1, q2 = torch.randn(b, A, generator=g) + 1.0, torch.randn(b, A, generator=g) + 1.0
    q2[::3] = q1[::3]
    return dict(kind="dsac", b=b, A=A, logits=logits, q1=q1, q2=q2,
                te=0.98 * math.log(max(A, 2)), nan_rows=(), floor=True), g


def plain_case(b, A):
    return _dsac_base(7000 + 10 * b + A, b, A)[0]


def _mask_patterns(A):
    """Boolean [A] masks, each leaving at least one entry: one entry, all but one, alternating
    (either parity), column 0, column A - 1, and at A >= 65 columns 63, 64 and both (either
    side of the boundary between a lane's first and second trip)."""
    one = lambda *cols: torch.zeros(A, dtype=torch.bool).index_fill_(  # noqa: E731
        0, torch.tensor(cols), True)
    even = torch.arange(A) % 2 == 0
    pats = [("one", one(A // 2)), ("all-but-one", ~one((2 * A) // 3)), ("even", even),
            ("odd", ~even), ("first", one(0)), ("last", one(A - 1))]
    if A >= 65:
        pats += [("col63", one(63)), ("col64", one(64)), ("col63+64", one(63, 64))]
    return pats


def masked_case(b, A, offset):
    """Every row masked by one of _mask_patterns(A), row i by pattern (i + offset) mod their
    number (so the one-row cases differ in pattern); at b = 65 every tenth row stays unmasked."""
    c, _ = _dsac_base(8000 + 10 * b + A, b, A)
    pats = _mask_patterns(A)
    used = []
    for i in range(b):
        if b == 65 and i % 10 == 9:
            continue
        name, m = pats[(i + offset) % len(pats)]
        c["logits"][i, m] = -INF
        used.append(name)
    c["patterns"] = used
    return c


def extreme_case(A):
    """Finite extremes (+-3e38: the normalised logit overflows f32's range), a spread of 1e4,
    rows of equal logits, and Q values of +-1e30 under masked entries (0 * 1e30: nothing may
    leak into V, the losses or the gradient).  Out of the floor, as loss_edges_common's
    "extreme": f32 rounds a normalised logit near -2e4 to 2e-3."""
    c, _ = _dsac_base(9000 + A, 9, A)
    x, q1, q2 = c["logits"], c["q1"], c["q2"]
    x[0, :6] = torch.tensor([3e38, -3e38, 0.0, 1.0, -1.0, 2.0])
    x[1] = -3e38
    x[1, 2] = 3e38
    x[2, :6] = torch.tensor([1e4, -1e4, 0.0, 1.0, -1.0, 2.0])
    x[3] = 1e4
    x[4] = -1e4
    x[5, 1] = -INF
    q1[5, 1] = q2[5, 1] = 1e30
    x[6, 0] = x[6, A - 1] = -INF
    q1[6, 0], q2[6, 0] = 1e30, 2e30
    q1[6, A - 1] = q2[6, A - 1] = -1e30
    c["floor"] = False
    return c


POISON_ROW = 37  # of 65: at A = 6 its 8-lane group shares a wave with seven other rows
POISONS = ("all-masked", "pos-inf", "nan")


def poison_case(kind, A):
    """(case, clean case): one row of all -inf, with one +inf logit or with one NaN logit; the
    reference is NaN in that row and in the losses.  The clean case has a plain row there."""
    clean, _ = _dsac_base(9500 + A, 65, A)
    c = dict(clean, logits=clean["logits"].clone(), nan_rows=(POISON_ROW,))
    if kind == "all-masked":
        c["logits"][POISON_ROW] = -INF
    else:
        c["logits"][POISON_ROW, A // 2] = INF if kind == "pos-inf" else NAN
    return c, clean


def _build_dsac():
    cases = {}
    for b, A in ((1, 2), (5, 18), (65, 6), (65, 130)):
        cases[f"plain-b{b}-A{A}"] = plain_case(b, A)
    for b in DSAC_BS:
        for k, A in enumerate(DSAC_AS):
            cases[f"masked-b{b}-A{A}"] = masked_case(b, A, k)
    for A in (6, 130):
        cases[f"extreme-A{A}"] = extreme_case(A)
        for kind in POISONS:
            c, clean = poison_case(kind, A)
            cases[f"poison-{kind}-A{A}"] = c
            cases[f"clean-A{A}"] = clean
    return cases


# -- C51 and QR -----------------------------------------------------------------------------------
DIST_OUTPUTS = ("loss", "vec", "grad")  # vec: the per-row cross-entropy (C51) / priority (QR)
WIDE_NS = (255, 256, 257, 513)  # one trip of a 256-thread workgroup, its edge, two and three
MAX_N = _C.DIST_MAX_N  # 4096
C51_KEYS = ("curr", "act", "next", "returns", "support", "weight")
QR_KEYS = ("curr", "act", "returns", "tau_hat", "weight")


def c51_case(b, A, N, weighted):
    c = dict(zip(C51_KEYS, c51_inputs(b, A, N, "cpu", weighted)))
    c.update(kind="c51", b=b, A=A, N=N, nan_rows=(), inf_rows=())
    return c


def qr_case(b, A, N, weighted):
    c = dict(zip(QR_KEYS, qr_inputs(b, A, N, "cpu", weighted)))
    c.update(kind="qr", b=b, A=A, N=N, nan_rows=(), inf_rows=())
    return c


def delta_z(N):
    return (V_MAX - V_MIN) / (N - 1)


def dist_args(case, dtype, device="cpu"):
    """The case's tensors in the order the reference and the kernel wrappers take them."""
    def cast(t):
        if t is None:
            return None
        return t.to(device=device, dtype=dtype if t.is_floating_point() else t.dtype).contiguous()
    return [cast(case[k]) for k in (C51_KEYS if case["kind"] == "c51" else QR_KEYS)]


def dist_batched(case, dtype, device="cpu"):
    """c51_reference / qr_reference on the whole batch."""
    args = dist_args(case, dtype, device)
    if case["kind"] == "c51":
        out = c51_reference(*args, V_MIN, V_MAX, delta_z(case["N"]))
    else:
        out = qr_reference(*args)
    return dict(zip(DIST_OUTPUTS, (t.detach().cpu() for t in out)))


def dist_rows(case, dtype, device="cpu"):
    """The same one batch row at a time: the loss is the mean of the rows' one-row losses and a
    row's gradient its one-row gradient over b."""
    args = dist_args(case, dtype, device)
    c51 = case["kind"] == "c51"
    batched = (0, 1, 2, 3, 5) if c51 else (0, 1, 2, 4)  # the arguments with a batch dimension
    b = case["b"]
    losses, vecs, grads = [], [], []
    for r in range(b):
        row = [a[r:r + 1] if i in batched and a is not None else a for i, a in enumerate(args)]
        if c51:
            loss, vec, grad = c51_reference(*row, V_MIN, V_MAX, delta_z(case["N"]))
        else:
            loss, vec, grad = qr_reference(*row)
        losses.append(loss.detach())
        vecs.append(vec.detach())
        grads.append(grad)
    out = (torch.stack(losses).sum() / b, torch.cat(vecs), torch.cat(grads) / b)
    return dict(zip(DIST_OUTPUTS, (t.cpu() for t in out)))


DIST_POISON_ROW = 1
DIST_POISONS = {"c51": ("nan-ret", "inf-ret", "nan-next", "zero-next"),
                "qr": ("nan-ret", "inf-ret")}


def dist_poison_case(kind, what):
    """b = 3, A = 3, N = 513, weighted; row 1 with NaN returns at one index below 256 and one
    above it, with a +inf and a -inf return, or with a NaN / two zeros in next (C51).  C51
    clamps the infinite returns to the support's ends and stays finite; QR's loss and that
    row's priority are +inf, as in torch."""
    c = (c51_case if kind == "c51" else qr_case)(3, 3, 513, True)
    r = DIST_POISON_ROW
    if what == "nan-ret":
        c["returns"][r, 100] = c["returns"][r, 300] = NAN
        c["nan_rows"] = (r,)
    elif what == "inf-ret":
        c["returns"][r, 5], c["returns"][r, 400] = INF, -INF
        if kind == "qr":
            c["inf_rows"] = (r,)
    elif what == "nan-next":
        c["next"][r, 7] = NAN
        c["nan_rows"] = (r,)
    else:
        c["next"][r, 7] = c["next"][r, 300] = 0.0
    return c


def _build_dist():
    cases = {}
    for kind, make in (("c51", c51_case), ("qr", qr_case)):
        for N in ((1,) if kind == "qr" else ()) + WIDE_NS:
            for A in (1, 3):
                for b in (1, 3):
                    for w in (0, 1):
                        cases[f"{kind}-b{b}-A{A}-N{N}-w{w}"] = make(b, A, N, bool(w))
        for A in (1, 3):  # the limit: 16 atoms per thread
            for w in (0, 1):
                cases[f"{kind}-b2-A{A}-N{MAX_N}-w{w}"] = make(2, A, MAX_N, bool(w))
        cases[f"{kind}-clean"] = make(3, 3, 513, True)
        for what in DIST_POISONS[kind]:
            cases[f"{kind}-{what}"] = dist_poison_case(kind, what)
    return cases


# -- tsrl_dist_select ------------------------------------------------------------------------------
SELECT_NS = (1, 255, 256, 257, 513, 4096, 5000)  # 5000: past the loss kernels' limit


def select_case(b, A, N, mode):
    """(sel, eval, w) with clear gaps between the actions' Q-values.  "qr": values of std 0.1
    around 0, 1, 2 in a shuffled order, reduced by their mean; "c51": probabilities tilted
    along the support by -0.1, 0 and 0.1 per unit, weighted by the support (N >= 2)."""
    g = torch.Generator().manual_seed(300000 * b + 3000 * A + N + (7 if mode == "qr" else 0))
    order = torch.stack([torch.randperm(A, generator=g) for _ in range(b)]).float()
    noise = torch.randn(b, A, N, generator=g)
    ev = torch.randn(b, A, N, generator=g)
    if mode == "qr":
        return 0.1 * noise + order.unsqueeze(-1), ev, None
    z = torch.linspace(V_MIN, V_MAX, N)
    tilt = 0.1 * (order - (A - 1) / 2).unsqueeze(-1) * z
    return (noise + tilt).softmax(-1), ev.softmax(-1), z


def _build_select():
    return {f"select-{mode}-b{b}-A{A}-N{N}": (b, A, N, mode)
            for mode in ("c51", "qr") for N in SELECT_NS for A in (1, 3) for b in (1, 3)
            if not (mode == "c51" and N == 1)}


DSAC_CASES = _build_dsac()
DIST_CASES = _build_dist()
SELECT_CASES = _build_select()
CASES = {**DSAC_CASES, **DIST_CASES}


def names(prefix, cases=None):
    return [n for n in (CASES if cases is None else cases) if n.startswith(prefix)]


def outputs(kind):
    return DSAC_OUTPUTS if kind == "dsac" else DIST_OUTPUTS


def ref_of(name, dtype, device="cpu"):
    case = CASES[name]
    return (dsac_ref if case["kind"] == "dsac" else dist_rows)(case, dtype, device)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """The f64 reference of a case, computed once on the CPU and left unchanged."""
    return ref_of(name, torch.float64)


def clean_rows(case):
    """[b] bool: the rows no poison touches."""
    keep = torch.ones(case["b"], dtype=torch.bool)
    keep[list(case["nan_rows"])] = False
    return keep


def case_err(case, got, want, o):
    """scaled_err of output ``o`` (tensors ``got`` and ``want``); a per-row output over the rows
    no poison touches (the poisoned rows are compared NaN for NaN)."""
    per_row = o in (DSAC_ROW_OUTPUTS if case["kind"] == "dsac" else ("vec", "grad"))
    return scaled_err(got, want, clean_rows(case) if per_row else None)


def floors(names_, r32_of):
    """Per (kind, output): the largest error of the torch-f32 formulation r32_of(name) against
    f64, scaled by max |ref|, over the cases that count towards the floor."""
    worst = {}
    for name in names_:
        case = CASES[name]
        if not case.get("floor", True):
            continue
        r64, r32 = ref64(name), r32_of(name)
        for o in outputs(case["kind"]):
            e = case_err(case, r32[o], r64[o], o)
            if math.isfinite(e):
                key = (case["kind"], o)
                worst[key] = max(worst.get(key, 0.0), e)
    return worst


def same_nans(got, want):
    """NaN in exactly the same entries."""
    return torch.equal(torch.isnan(got.detach().cpu()), torch.isnan(want))
