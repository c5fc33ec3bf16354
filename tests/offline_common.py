"""References and case lists shared by tests/test_offline_host.py and tests/test_gpu_offline.py:
the reference's formulas (tianshou/policy/imitation/discrete_{bcq,cql,crr}.py) on torch f64 with
autograd -- the judge of the fused kernels' analytic gradients -- a NumPy f32 restatement of
the BCQ action test, seeded inputs, and the policies of tests/golden/offline.npz (tools/
gen_goldens.py gen_offline: the reference's policies on CPU torch)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

BS = (1, 63, 64, 65, 257)      # lane, wave, workgroup and multi-partial edges
AS = (1, 2, 18, 65)
NS = (2, 63, 64, 65, 200)
KINDS = ("random", "ties", "spread")
CRR = dict(gamma=0.9, beta=2.0, ub=3.0, mqw=0.7)


def table(kind, b, A, seed):
    """[b, A] f32: gaussian, a few distinct values (ties), or rows spread over 1e4 so that a
    logsumexp without max-subtraction overflows."""
    g = np.random.default_rng(seed)
    if kind == "ties":
        return g.integers(-2, 3, (b, A)).astype(np.float32) * 0.5
    x = g.normal(size=(b, A)).astype(np.float32)
    return x * np.float32(2500.0) if kind == "spread" else x


def select_ref(q, logits, log_tau, q_eval, paper):
    """discrete_bcq.py:97-99 in NumPy f32.  Reference mode: the first allowed action (what the
    reference's NaN-producing line returns); paper mode: torch's argmax over the allowed Q."""
    with np.errstate(invalid="ignore"):
        ratio = logits - torch.as_tensor(logits).max(-1, keepdim=True).values.numpy()
    allowed = ~(ratio < np.float32(log_tau))
    if paper:
        masked = torch.as_tensor(np.where(allowed, q, -np.inf).astype(np.float32))
        act = masked.argmax(-1).numpy()
    else:
        act = allowed.argmax(-1)
    return act, q_eval[np.arange(len(act)), act]


def _leaf(x):
    return torch.as_tensor(x, dtype=torch.float64).requires_grad_()


def bcq_ref(q, logits, act, returns, weight_reg):
    """(loss, q, i, reg), grad_q, grad_logits."""
    q, l = _leaf(q), _leaf(logits)
    a = torch.as_tensor(act)
    q_loss = F.smooth_l1_loss(q[torch.arange(len(a)), a], torch.as_tensor(returns).double())
    i_loss = F.nll_loss(F.log_softmax(l, -1), a)
    reg = l.pow(2).mean()
    loss = q_loss + i_loss + weight_reg * reg
    loss.backward()
    return torch.stack([loss, q_loss, i_loss, reg]).detach().numpy(), q.grad.numpy(), \
        l.grad.numpy()


def cql_ref(curr, act, returns, tau_hat, weight, mqw):
    """(loss, qr, cql), grad [b, A, N], prio [b]."""
    x = _leaf(curr)
    a = torch.as_tensor(act)
    cd = x[torch.arange(len(a)), a, :].unsqueeze(2)
    td = torch.as_tensor(returns).double().unsqueeze(1)
    diff = F.smooth_l1_loss(td, cd, reduction="none")
    tau = torch.as_tensor(tau_hat).double().view(1, -1, 1)
    huber = (diff * (tau - (td - cd).detach().le(0.).double()).abs()).sum(-1).mean(1)
    w = 1.0 if weight is None else torch.as_tensor(weight).double()
    qr = (huber * w).mean()
    q = x.mean(2)
    cql = q.logsumexp(1).mean() - q.gather(1, a.unsqueeze(1)).mean()
    loss = qr + mqw * cql
    loss.backward()
    return torch.stack([loss, qr, cql]).detach().numpy(), x.grad.numpy(), \
        diff.detach().abs().sum(-1).mean(1).numpy()


def crr_ref(q, logits, act, t_logits, t_q, rew, done, mode, gamma, beta, ub, mqw):
    """(loss, actor, critic, cql), grad_q, grad_logits, advantage / beta, exp(advantage / beta)."""
    q, l = _leaf(q), _leaf(logits)
    a = torch.as_tensor(act)
    qa = q.gather(1, a.unsqueeze(1))
    tp = torch.softmax(torch.as_tensor(t_logits).double(), -1)
    ev = (torch.as_tensor(t_q).double() * tp).sum(-1, keepdim=True)
    ev[torch.as_tensor(done) > 0] = 0.0
    target = torch.as_tensor(rew).double().unsqueeze(1) + gamma * ev
    critic = 0.5 * F.mse_loss(qa, target)
    dist = torch.distributions.Categorical(logits=l)
    adv = qa - (q * dist.probs).sum(-1, keepdim=True)
    if mode == "binary":
        coef = (adv > 0).double()
    elif mode == "exp":
        coef = (adv / beta).exp().clamp(0, ub)
    else:
        coef = 1.0
    actor = (-dist.log_prob(a) * coef).mean()
    cql = (q.logsumexp(1) - qa.flatten()).mean()
    loss = actor + critic + mqw * cql
    loss.backward()
    z = (adv / beta).detach().numpy().ravel()
    return torch.stack([loss, actor, critic, cql]).detach().numpy(), q.grad.numpy(), \
        l.grad.numpy(), z, np.exp(z)


# seeds other than 0, chosen on crr_ref alone (test_offline_host.py asserts the margins)
CRR_SEEDS = {("spread", 257, 2): 1, ("spread", 257, 65): 1}


def crr_case(kind, b, A):
    """Inputs of one CRR case.  Q-values within a few units, so |adv / beta| stays far below
    80 and no advantage is zero by a tie; "ties" and "spread" apply to the two logits tables.
    Some rows done."""
    seed = CRR_SEEDS.get((kind, b, A), 0)
    g = np.random.default_rng(1000 * b + A + seed)
    return dict(q=table("random", b, A, seed + 1) * np.float32(1.5),
                logits=table(kind, b, A, seed + 2), act=g.integers(0, A, b),
                t_logits=table(kind, b, A, seed + 3), t_q=table("random", b, A, seed + 4),
                rew=g.normal(size=b).astype(np.float32),
                done=(g.random(b) < 0.3).astype(np.uint8))


def crr_margins_ok(z, e, mode, beta, ub):
    """The margins the CRR cases keep from the kernel's two decision points: the coefficient
    1e-3 relative off the bound (exp), the advantage 1e-4 off zero unless it is exactly zero,
    as with one action (binary); |adv / beta| < 80 always."""
    if not np.all(np.abs(z) < 80):
        return False
    if mode == "exp":
        return bool(np.all(np.abs(e - ub) > 1e-3 * ub))
    if mode == "binary":
        adv = z * beta
        return bool(np.all((adv == 0) | (np.abs(adv) > 1e-4)))
    return True


# -- the recording ------------------------------------------------------------------------------
def recording(golden_dir):
    z = np.load(os.path.join(golden_dir, "offline.npz"))
    return z, json.loads(str(z["cfg"]))


def make_policy(z, cfg, tag, dev="cpu", **attrs):
    """The variant's policy over this package's networks, the recorded initial state_dict
    (the reference's checkpoint) loaded with strict=True."""
    from tianshou_amd import policy as P
    from tianshou_amd.utils.net import DiscreteActor, DiscreteCritic, Net
    v, D, A, H = cfg["variants"][tag], cfg["D"], cfg["A"], cfg["hidden"]
    if v["kind"] == "cql":
        nets = [Net(D, A, hidden_sizes=(H, H), num_atoms=cfg["N"], device=dev)]
    else:
        t1 = Net(D, hidden_sizes=(H, H), device=dev)
        t2 = t1 if v.get("shared") else Net(D, hidden_sizes=(H, H), device=dev)
        second = DiscreteCritic(t2, hidden_sizes=[H], last_size=A, device=dev) \
            if v["kind"] == "crr" else \
            DiscreteActor(t2, A, hidden_sizes=[H], softmax_output=False, device=dev)
        nets = [DiscreteActor(t1, A, hidden_sizes=[H], softmax_output=False, device=dev), second]
    params = list({id(p): p for n in nets for p in n.parameters()}.values())
    optim = torch.optim.RMSprop(params, lr=7e-4, eps=1e-5, alpha=0.99) if v["optim"] == "rms" \
        else torch.optim.Adam(params, lr=1e-3)
    if v["kind"] == "bcq":
        policy = P.DiscreteBCQPolicy(nets[0], nets[1], optim, cfg["gamma"], v["n_step"], v["freq"],
                                     unlikely_action_threshold=cfg["tau"])
    elif v["kind"] == "cql":
        policy = P.DiscreteCQLPolicy(nets[0], optim, cfg["gamma"], cfg["N"], v["n_step"],
                                     v["freq"], min_q_weight=cfg["mqw"])
    else:
        policy = P.DiscreteCRRPolicy(nets[0], nets[1], optim, cfg["gamma"], v["mode"], cfg["ub"],
                                     cfg["beta"], cfg["mqw"], v["freq"], action_scaling=False,
                                     deterministic_eval=True)
        policy.action_type = "discrete"
    policy.load_state_dict(state(z, f"{tag}_init_sd_"), strict=True)
    policy.to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy


def state(z, prefix):
    return {k[len(prefix):]: torch.as_tensor(z[k]) for k in z.files if k.startswith(prefix)}


def state_dev(policy, z, prefix):
    """max |parameter - recorded| over the whole state_dict (online and target networks)."""
    want = state(z, prefix)
    sd = policy.state_dict()
    assert list(sd) == list(want)
    return max(float((sd[k].detach().cpu().double() - want[k].double()).abs().max()) for k in sd)


def assert_state(policy, z, prefix, tag):
    """Adam parameters, online and target: rtol 1e-5 / atol 1e-6."""
    for k, t in policy.state_dict().items():
        np.testing.assert_allclose(t.detach().cpu().numpy(), z[prefix + k], rtol=1e-5, atol=1e-6,
                                   err_msg=f"{tag} {k}")
