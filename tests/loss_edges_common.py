"""Cases and references shared by tests/test_gpu_loss_edges.py (the PPO / A2C loss kernels of
csrc/ppo.hip, csrc/ppo_cat.hip and csrc/ppo_loss.h at masked logits, extreme logits,
unnormalised probabilities, the width limits, Gaussian edge inputs and b_global != b) and
tests/test_loss_edges_host.py (which checks these references against each other on the CPU).

One reference function, ``loss_ref(case, dtype)``, states the minibatch loss of
tianshou/policy/modelfree/ppo.py:106-151 and a2c.py:126-137 in torch: at float64 it is the
reference (the ratio stays in f64), at float32 it is the torch-f32 formulation, which for the
PPO objective with b_global == B is oracle.ref.ppo_categorical_loss_torch /
ppo_gaussian_loss_torch operation for operation (the host test compares the two).

The Categorical distribution is written out (``cat_dist``) as torch.distributions.Categorical
computes it, with float32's constants at either precision: the clamp of the probabilities at
eps = 2^-23 and of the logits at float32's lowest value are part of the operation the kernel
implements for f32 inputs, not rounding; torch's own f64 Categorical would clamp at 2^-52 and
give log(0-probability) = -36 where the f32 operation gives -15.9.
"""
import functools

import numpy as np
import torch
from torch.distributions import Independent, Normal

F32_EPS = float(torch.finfo(torch.float32).eps)
F32_MIN = float(torch.finfo(torch.float32).min)
INF = float("inf")


def cat_dist(x, mode):
    """(normalised logits, probs, per-row entropy) of Categorical(logits=x) (mode 0) or
    Categorical(probs=x) (mode 1): torch/distributions/categorical.py and utils.py."""
    if mode == 0:
        logits = x - x.logsumexp(dim=-1, keepdim=True)
        probs = torch.softmax(logits, dim=-1)
    else:
        probs = x / x.sum(-1, keepdim=True)
        logits = torch.log(probs.clamp(min=F32_EPS, max=1 - F32_EPS))
    ent = -(torch.clamp(logits, min=F32_MIN) * probs).sum(-1)
    return logits, probs, ent


def loss_ref(case, dtype, device="cpu"):
    """The loss of one case at ``dtype``, computed on ``device``.  Returns a dict: the four terms, the gradients, the
    per-row log-prob, and ``rows``: the per-row outcomes of every comparison the loss branches
    on (a row whose outcomes differ between f32 and f64 is branch-ambiguous)."""
    p, kind, B = case["p"], case["kind"], case["B"]
    cast = lambda k: case[k].detach().to(device=device, dtype=dtype).clone()  # noqa: E731
    value = cast("value").requires_grad_(True)
    if kind == "cat":
        x = cast("x").requires_grad_(True)
        logits, _, ent_rows = cat_dist(x, case["mode"])
        logp = logits.gather(-1, case["act"].to(device).unsqueeze(-1)).squeeze(-1)
        leaves = dict(grad_x=x, grad_value=value)
    else:
        mu = cast("mu").requires_grad_(True)
        ls = cast("log_std").requires_grad_(True)
        sigma = (ls.view(1, -1) + torch.zeros_like(mu)).exp()
        dist = Independent(Normal(mu, sigma), 1)
        logp = dist.log_prob(cast("act"))
        ent_rows = dist.entropy()
        leaves = dict(grad_mu=mu, grad_ls=ls, grad_value=value)
    n = p["b_global"]
    # the mean over the (global) minibatch: this process's rows over the global count
    mean_ = (lambda t: t.mean()) if n == B else (lambda t: t.sum() / n)  # noqa: E731
    adv = cast("adv")
    if p["norm_adv"]:
        pop = case["adv_pop"].to(device=device, dtype=dtype) if "adv_pop" in case else adv
        if pop.numel() == 1:
            # torch's unbiased std of one value is NaN; the kernels take that variance as 0 and
            # the normalised advantage is (adv - adv) / (0 + 1e-8) = 0.  The reference states
            # that value, as tests/test_gpu_mlp_bwd.py's does for the fused tail
            adv = adv * 0
        else:
            adv = (adv - pop.mean()) / (pop.std() + 1e-8)
    eps = p["eps_clip"]
    c = lambda v: torch.tensor(v, dtype=dtype, device=device)  # noqa: E731
    rows = [torch.sign(adv)]
    if p["objective"] == "a2c":
        clip = -mean_(logp * adv)
    else:
        ratio = (logp - cast("logp_old")).exp()
        if dtype == torch.float32:
            ratio = ratio.float()
        surr1 = ratio * adv
        surr2 = ratio.clamp(1.0 - eps, 1.0 + eps) * adv
        clip1 = torch.min(surr1, surr2)
        rows += [torch.sign(ratio - c(1.0 - eps)), torch.sign(ratio - c(1.0 + eps)),
                 torch.sign(surr1 - surr2)]
        if p["dual_clip"]:
            clip2 = torch.max(clip1, p["dual_clip"] * adv)
            clip = -mean_(torch.where(adv < 0, clip2, clip1))
            rows.append(torch.sign(clip1 - p["dual_clip"] * adv) * (adv < 0))
        else:
            clip = -mean_(clip1)
    ret, v_s = cast("ret"), cast("v_s")
    if p["value_clip"]:
        dlt = value - v_s
        v_clip = v_s + dlt.clamp(-eps, eps)
        vf1, vf2 = (ret - value).pow(2), (ret - v_clip).pow(2)
        vf = mean_(torch.max(vf1, vf2))
        rows += [torch.sign(vf1 - vf2), torch.sign(dlt + c(eps)), torch.sign(dlt - c(eps))]
    else:
        vf = mean_((ret - value).pow(2))
    # every row of the Gaussian has the same entropy, which the kernel states once
    ent = ent_rows.mean() if kind == "gauss" else mean_(ent_rows)
    loss = clip + p["vf_coef"] * vf - p["ent_coef"] * ent
    grads = torch.autograd.grad(loss, list(leaves.values()))
    out = dict(loss=loss, clip=clip, vf=vf, ent=ent, logp=logp)
    out.update(zip(leaves, grads))
    out = {k: v.detach().cpu() for k, v in out.items()}
    out["rows"] = torch.stack([r.detach().to(torch.float64) for r in rows]).cpu()
    return out


def ambiguous(r64, r32):
    """Rows on which the two evaluations decide one of the loss's comparisons differently."""
    a, b = r64["rows"], r32["rows"]
    return ((a != b) & ~(torch.isnan(a) & torch.isnan(b))).any(0)


@functools.lru_cache(maxsize=None)
def refs(name):
    """(f64 reference, torch-f32 formulation, ambiguous-row mask) of a case, computed once."""
    case = CASES[name]
    r64, r32 = loss_ref(case, torch.float64), loss_ref(case, torch.float32)
    return r64, r32, ambiguous(r64, r32)


TERMS = ("loss", "clip", "vf", "ent")
ROW_GRADS = ("grad_x", "grad_mu", "grad_value")  # one row of the gradient per minibatch row


def outputs(kind):
    return TERMS + (("grad_x",) if kind == "cat" else ("grad_mu", "grad_ls")) + \
        ("grad_value", "logp")


def scaled_err(got, ref64, keep=None):
    """max |got - ref| / max |ref| over the rows in ``keep`` (all by default).  An entry that
    is NaN (or the same infinity) in both counts as equal; NaN against a number is inf."""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    if keep is not None and got.dim() >= 1 and got.shape[0] == keep.shape[0]:
        got, ref64 = got[keep], ref64[keep]
    if got.numel() == 0:
        return 0.0
    same = (torch.isnan(got) & torch.isnan(ref64)) | (got == ref64)
    diff = torch.where(same, torch.zeros_like(ref64), (got - ref64).abs())
    if bool(torch.isnan(diff).any()):
        return INF
    fin = ref64[torch.isfinite(ref64)]
    scale = float(fin.abs().max()) if fin.numel() else 0.0
    return float(diff.max()) / (scale or 1.0)


def check_ambiguous_rows(got, r32, amb, name):
    """Branch-ambiguous rows: the gradient against the torch-f32 formulation alone."""
    if not bool(amb.any()):
        return
    want = r32[name]
    np.testing.assert_allclose(got.detach().cpu().numpy()[amb.numpy()], want.numpy()[amb.numpy()],
                               rtol=1e-4, atol=1e-6 * float(want.abs().max()) + 1e-9)


def floors(names, refs_of=refs):
    """Per (kind, output): the largest error of the torch-f32 formulation against f64, scaled
    by max |ref|, over the cases that count towards the floor.  refs_of(name) gives a case's
    (f64 reference, torch-f32 formulation, ambiguous rows)."""
    worst = {}
    for name in names:
        case = CASES[name]
        if not case.get("floor", True):
            continue
        r64, r32, amb = refs_of(name)
        for o in outputs(case["kind"]):
            e = scaled_err(r32[o], r64[o], ~amb if o in ROW_GRADS else None)
            if np.isfinite(e):
                key = (case["kind"], o)
                worst[key] = max(worst.get(key, 0.0), e)
    return worst


# -- case builders ------------------------------------------------------------------------------
PPO = dict(objective="ppo", eps_clip=0.2, dual_clip=0.0, value_clip=False, norm_adv=False,
           vf_coef=0.25, ent_coef=0.01)


def _base(seed, kind, B, A, mode=0, **p):
    g = torch.Generator().manual_seed(seed)
    c = dict(kind=kind, B=B, A=A, mode=mode, p=dict(PPO, b_global=B, **p))
    c["value"] = torch.randn(B, generator=g)
    c["adv"] = torch.randn(B, generator=g) * 2 + 0.3
    c["ret"] = torch.randn(B, generator=g)
    c["v_s"] = c["ret"] + torch.randn(B, generator=g) * 0.3
    if kind == "cat":
        z = torch.randn(B, A, generator=g) * 1.5
        c["x"] = z if mode == 0 else torch.softmax(z, -1)
        c["act"] = torch.randint(0, A, (B,), generator=g)
    else:
        c["mu"] = torch.randn(B, A, generator=g)
        c["log_std"] = torch.randn(A, generator=g) * 0.3 - 0.5
        c["act"] = c["mu"] + c["log_std"].exp() * torch.randn(B, A, generator=g)
    return c, g


def _finish(c, g):
    """logp_old near the f32 log-prob of the finished inputs, so that the ratio straddles the
    clip range; a row without a finite log-prob (masked or invalid action) gets -1."""
    if c["kind"] == "cat":
        act = c["act"].clamp(0, c["A"] - 1)
        lp = cat_dist(c["x"], c["mode"])[0].gather(-1, act.unsqueeze(-1)).squeeze(-1)
    else:
        sigma = c["log_std"].exp().view(1, -1).expand_as(c["mu"])
        lp = Independent(Normal(c["mu"], sigma), 1).log_prob(c["act"])
    lp = torch.where(torch.isfinite(lp), lp, torch.full_like(lp, -1.0))
    c["logp_old"] = lp + torch.randn(c["B"], generator=g) * 0.2
    return c


def masked_case(B, A, ent_coef, objective):
    """Test 1: 1 .. A-1 entries of -inf in every second row, every count of masked entries in
    a row whose taken action is unmasked; under the PPO objective the last row's taken action
    is masked (log-prob -inf, ratio 0, finite loss; under A2C that row's term -log_prob * adv
    is infinite, in torch as in the kernel, so A2C gets no such row)."""
    c, g = _base(1000 * B + 10 * A + (objective == "a2c"), "cat", B, A, 0,
                 ent_coef=ent_coef, objective=objective)
    counts = []
    for i in range(0, B, 2):
        k = 1 + (i // 2) % (A - 1)
        order = torch.randperm(A, generator=g)
        c["x"][i, order[:k]] = -INF
        c["act"][i] = order[k + int(torch.randint(0, A - k, (1,), generator=g))]
        counts.append(k)
    c["masked_counts"] = counts
    if objective == "ppo":
        c["x"][B - 1, 0] = -INF
        c["x"][B - 1, 1] = 0.5
        c["act"][B - 1] = 0
        c["masked_taken"] = B - 1
    return _finish(c, g)


def extreme_case():
    """Test 2: rows with +-90 and +-1e4 (probabilities that underflow, normalised logits near
    -2e4) and rows of equal logits, among random rows."""
    c, g = _base(2, "cat", 65, 6, 0)
    x = c["x"]
    x[0] = torch.tensor([90.0, -90.0, 0.0, 1.0, -1.0, 2.0])
    x[1] = torch.tensor([1e4, -1e4, 0.0, 1.0, -1.0, 2.0])
    x[2] = torch.tensor([-1e4, 1e4, 1e4, 0.0, 90.0, -90.0])
    x[3] = 3.7
    x[4] = 0.0
    x[5] = -1e4
    x[6] = 1e4
    x[7] = torch.tensor([-90.0, -90.0, -90.0, -90.0, -90.0, 90.0])
    c["act"][:8] = torch.tensor([1, 1, 0, 2, 5, 0, 3, 0])
    c["floor"] = False  # f32 rounds a log-prob near -2e4 to 2e-3: not the other cases' floor
    return _finish(c, g)


def one_action_case():
    """Test 2: A = 1, where log-prob, entropy and the gradient are exactly 0."""
    c, g = _base(3, "cat", 65, 1, 0)
    return _finish(c, g)


PAIRS = 64  # rows [PAIRS, 2 * PAIRS) of probs_case are rows [0, PAIRS) times 3


def probs_case(ent_coef):
    """Test 3: Categorical(probs=x) with rows that do not sum to 1: x = c * softmax(z), c per
    row from {1, 3, 0.25, 1e-3}; rows with exact zeros; a one-hot row times 3.  Rows
    [PAIRS, 2 PAIRS) repeat rows [0, PAIRS) (c = 1) with c = 3 and the same act, logp_old and
    adv.  The taken action never has probability 0: there log_prob is log(eps), and eps
    belongs to the number format."""
    B, A = 257, 6
    c, g = _base(4, "cat", B, A, 1, ent_coef=ent_coef)
    x = c["x"]
    # (the low 8 mantissa bits cleared, so that 3 * x is exact in f32)
    x[:PAIRS] = (x[:PAIRS].view(torch.int32) & ~0xFF).view(torch.float32)
    x[PAIRS:2 * PAIRS] = x[:PAIRS]
    for k in ("act", "adv"):
        c[k][PAIRS:2 * PAIRS] = c[k][:PAIRS]
    scale = torch.tensor([0.25, 1.0, 3.0, 1e-3])[torch.arange(B) % 4]
    scale[:PAIRS] = 1.0
    scale[PAIRS:2 * PAIRS] = 3.0
    for i in range(2 * PAIRS, 2 * PAIRS + 12):  # exact zeros, the taken action kept
        drop = torch.randperm(A, generator=g)[:1 + i % (A - 1)]
        x[i, drop] = 0.0
        x[i, c["act"][i]] = max(float(x[i, c["act"][i]]), 0.125)
    c["x"] = x * scale.unsqueeze(-1)
    hot = 2 * PAIRS + 12
    c["x"][hot] = 0.0
    c["x"][hot, 2] = 3.0
    c["act"][hot] = 2
    _finish(c, g)
    c["logp_old"][PAIRS:2 * PAIRS] = c["logp_old"][:PAIRS]
    return c


WIDTHS = (1, 31, 32, 33, 63, 64)
WIDTH_ROWS = (1, 255, 256, 257)


def width_case(kind, B, A):
    """Test 4: the widths around 64 KiB of LDS and at the 128 KiB maximum, ragged and exact
    blocks, advantage normalisation and value clip on.  (B = 1: see loss_ref on the std of one
    advantage.)"""
    c, g = _base(5000 + 100 * B + A + (kind == "cat"), kind, B, A, 0, norm_adv=True,
                 value_clip=True)
    return _finish(c, g)


def gauss_edge_case():
    """Test 6: log_std in {-5, 0, 2}; rows with act == mu exactly; rows 8 sigma away."""
    c, g = _base(6, "gauss", 257, 3, dual_clip=3.0, value_clip=True)
    c["log_std"] = torch.tensor([-5.0, 0.0, 2.0])
    sig = c["log_std"].exp()
    c["act"] = c["mu"] + sig * torch.randn(257, 3, generator=g)
    c["act"][:16] = c["mu"][:16]
    c["act"][16:24] = c["mu"][16:24] + 8.0 * sig
    c["act"][24:32] = c["mu"][24:32] - 8.0 * sig * torch.tensor([1.0, 0.0, 0.0])
    c["act"][32:40] = c["mu"][32:40] + 8.0 * sig * torch.tensor([0.0, 0.0, 1.0])
    c["exact_rows"] = 16
    return _finish(c, g)


def global_case(kind):
    """Test 7: this process holds 257 rows of a 771-row global minibatch: every third
    advantage of the population, whose moments normalise them."""
    B, N = 257, 771
    c, g = _base(7 + (kind == "cat"), kind, B, 6 if kind == "cat" else 3, 0, norm_adv=True,
                 value_clip=True)
    c["adv_pop"] = torch.randn(N, generator=g) * 2 + 0.3
    c["adv"] = c["adv_pop"][::3].clone()
    c["p"]["b_global"] = N
    return _finish(c, g)


def shifted_adv_case():
    """Test 8: advantages with mean 1e4 and std 1 through a loss launch with norm_adv.  f32
    moments of such values are poor (torch's mean alone is off by ~1e-3 of the std), so this
    case stays out of the floor."""
    c, g = _base(8, "cat", 257, 6, 0, norm_adv=True)
    c["adv"] = torch.randn(257, generator=g) + 1e4
    c["floor"] = False
    return _finish(c, g)


def _build():
    cases = {}
    for B in (65, 257):
        for A in (2, 6, 18):
            for ent in (0.0, 0.01):
                for obj in ("ppo", "a2c"):
                    cases[f"masked-{obj}-B{B}-A{A}-ent{ent}"] = masked_case(B, A, ent, obj)
    cases["extreme"] = extreme_case()
    cases["one-action"] = one_action_case()
    for ent in (0.0, 0.01):
        cases[f"probs-ent{ent}"] = probs_case(ent)
    for kind in ("cat", "gauss"):
        for A in WIDTHS:
            for B in WIDTH_ROWS:
                cases[f"width-{kind}-B{B}-A{A}"] = width_case(kind, B, A)
    cases["gauss-edge"] = gauss_edge_case()
    for kind in ("cat", "gauss"):
        cases[f"global-{kind}"] = global_case(kind)
    cases["shifted-adv"] = shifted_adv_case()
    return cases


CASES = _build()


def names(prefix):
    return [n for n in CASES if n.startswith(prefix)]


# -- learn-level helpers (tests/test_gpu_ppo_discrete.py, test_gpu_a2c.py, test_gpu_ppo.py) ------
MASKED_ACTIONS = (1, 4)


class MaskedActor(torch.nn.Module):
    """Net(8 -> 64, 64), a 6-way head, and -inf over actions {1, 4} wherever obs[:, 0] > 0:
    the usual way to rule out illegal actions.  The mask is added (log of a 0 / 1 legality
    mask), so the head receives the loss's gradient at the masked entries as it is: a NaN
    there reaches every parameter, where masked_fill's backward would drop it."""

    def __init__(self, dev):
        super().__init__()
        from tianshou_amd.utils.net import Net
        self.net = Net(8, hidden_sizes=(64, 64), device=dev)
        self.head = torch.nn.Linear(64, 6)
        self.register_buffer("illegal", torch.zeros(6, dtype=torch.bool))
        self.illegal[list(MASKED_ACTIONS)] = True

    def forward(self, obs, state=None, info={}):
        h, _ = self.net(obs, state)
        legal = ~((obs[:, :1] > 0) & self.illegal)
        return self.head(h) + legal.float().log(), state


def cat_logits(x):
    return torch.distributions.Categorical(logits=x)


def discrete_policy(cls, dev, actor, n_act, seed, **kw):
    """(policy, twin) of ``cls`` over ``actor`` and a DiscreteCritic: the same weights, each
    with its own Adam."""
    import copy
    from tianshou_amd.env import Discrete
    from tianshou_amd.utils.net import ActorCritic, DiscreteCritic, Net
    torch.manual_seed(seed)
    actor = actor().to(dev)
    critic = DiscreteCritic(Net(8, hidden_sizes=(64, 64), device=dev), device=dev).to(dev)
    out = []
    for a, c in ((actor, critic), (copy.deepcopy(actor), copy.deepcopy(critic))):
        optim = torch.optim.Adam(ActorCritic(a, c).parameters(), lr=1e-3)
        out.append(cls(a, c, optim, cat_logits, action_space=Discrete(n_act),
                       max_grad_norm=0.5, vf_coef=0.5, ent_coef=0.01, action_scaling=False,
                       **kw).to(dev))
    return out


def discrete_batch(policy, dev, n, n_act, seed, illegal=()):
    """n rows for learn(): random obs, actions that are legal in their row, logp_old near
    the policy's own log-prob."""
    from tianshou_amd.data import Batch
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, 8, generator=g)
    act = torch.randint(0, n_act, (n,), generator=g)
    legal = torch.tensor([a for a in range(n_act) if a not in illegal])
    masked_row = obs[:, 0] > 0
    act[masked_row] = legal[torch.randint(0, len(legal), (int(masked_row.sum()),), generator=g)]
    ret = torch.randn(n, generator=g)
    b = Batch(obs=obs.to(dev), act=act.to(dev), adv=torch.randn(n, generator=g).to(dev),
              returns=ret.to(dev), v_s=(ret + 0.3 * torch.randn(n, generator=g)).to(dev))
    with torch.no_grad():
        lp = cat_logits(policy.actor(b.obs)[0]).log_prob(b.act)
    assert bool(torch.isfinite(lp).all())
    b.logp_old = lp + 0.1 * torch.randn(n, generator=g).to(dev)
    return b


def count_calls(policy, name):
    """Wrap policy.<name> to count its calls; returns the list the calls are appended to."""
    calls, fn = [], getattr(policy, name)

    def wrapped(*a, **kw):
        calls.append(name)
        return fn(*a, **kw)
    setattr(policy, name, wrapped)
    return calls


def filled_buffer(dev, E, T, obs_dim, act_of, seed):
    """A VectorReplayBuffer of E envs x T steps of random transitions; act_of(rng, E) draws
    one step's actions."""
    from tianshou_amd.data import Batch, VectorReplayBuffer
    rng = np.random.RandomState(seed)
    buf = VectorReplayBuffer(E * T, E, device=dev)
    for _ in range(T):
        buf.add(Batch(obs=rng.randn(E, obs_dim).astype(np.float32), act=act_of(rng, E),
                      rew=rng.randn(E), terminated=rng.rand(E) < 0.1,
                      truncated=np.zeros(E, bool),
                      obs_next=rng.randn(E, obs_dim).astype(np.float32)),
                buffer_ids=np.arange(E))
    return buf


def state_of(policy):
    return {k: v.detach().cpu().clone() for k, v in policy.state_dict().items()}


def compare_runs(res, res_twin, sd, sd_twin, keys, loss_tol, param_tol, what):
    """Losses and parameters of a run and its twin at (rtol, atol) each; prints the maxima."""
    worst_l = max(float(np.abs(np.asarray(res[k]) - np.asarray(res_twin[k])).max())
                  for k in keys)
    worst_p = max(float((sd[k].double() - sd_twin[k].double()).abs().max()) for k in sd)
    print(f"{what}: max |loss - twin| {worst_l:.3g}, max |param - twin| {worst_p:.3g}")
    assert all(bool(torch.isfinite(v).all()) for v in sd.values()), "non-finite parameter"
    for k in keys:
        np.testing.assert_allclose(res[k], res_twin[k], rtol=loss_tol[0], atol=loss_tol[1],
                                   err_msg=k)
    for k in sd:
        np.testing.assert_allclose(sd[k].numpy(), sd_twin[k].numpy(), rtol=param_tol[0],
                                   atol=param_tol[1], err_msg=k)
