"""Shared by tests/test_dsac_host.py and tests/test_gpu_dsac.py: reading tests/golden/dsac.npz
(tools/gen_goldens.py gen_dsac), building the nets, optimisers and policies its variants name,
and the plain f64 NumPy restatement of the three kernels of csrc/dsac.hip.  Every recorded
quantity of a variant is one array, the six updates stacked."""
import json
import os

import numpy as np
import torch

from tests.sac_common import loss_keys  # noqa: F401  (re-exported)

TAGS = ["dsac", "dsac_auto", "dsac_per", "dsac_rms", "dsac_softmax"]
ADAM_TAGS = [t for t in TAGS if t != "dsac_rms"]
N_UPDATES = 6
_CACHE = {}


def golden(golden_dir):
    z = _CACHE.get(golden_dir)
    if z is None:
        with np.load(os.path.join(golden_dir, "dsac.npz")) as f:
            z = _CACHE[golden_dir] = {k: f[k] for k in f.files}
    return z


def learn_cfg(z):
    return json.loads(str(z["learn_cfg"]))


def make_optim(kind, params, lr=None, adam_eps=1e-5):
    """gen_dsac's optimisers: Adam at eps 1e-5 (learn_cfg's ``adam_eps``; the generator says
    why), RMSprop as every recording's, SGD for the fall-back tests."""
    if kind == "rms":
        return torch.optim.RMSprop(params, lr=lr or 7e-4, eps=1e-5, alpha=0.99)
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr or 1e-2)
    return torch.optim.Adam(params, lr=lr or 1e-3, eps=adam_eps)


def build_nets(D, A, hidden, softmax, dev):
    from tianshou_amd.utils.net import DiscreteActor, DiscreteCritic, Net
    actor = DiscreteActor(Net(D, hidden_sizes=hidden, device=dev), (A,), softmax_output=softmax,
                          device=dev).to(dev)
    critics = [DiscreteCritic(Net(D, hidden_sizes=hidden, device=dev), last_size=A,
                              device=dev).to(dev) for _ in range(2)]
    return dict(actor=actor, critic1=critics[0], critic2=critics[1])


def make_nets(z, cfg, v, dev):
    """{name: module} of variant ``v`` with the recorded initial weights."""
    nets = build_nets(cfg["D"], cfg["A"], tuple(cfg["hidden"]), bool(v.get("softmax")), dev)
    with torch.no_grad():
        for name, net in nets.items():
            for k, p in net.named_parameters():
                p.copy_(torch.as_tensor(z[f"init_{name}.{k}"]))
    return nets


def make_policy(z, cfg, tag, dev, optim=None, alpha_kind=None, **attrs):
    from tianshou_amd.policy import DiscreteSACPolicy
    v = cfg["variants"][tag]
    nets = make_nets(z, cfg, v, dev)
    eps = cfg["adam_eps"]
    opt = {n: make_optim(optim or v["optim"], m.parameters(), adam_eps=eps)
           for n, m in nets.items()}
    alpha = cfg["alpha"]
    if v["auto"]:
        log_alpha = torch.zeros(1, requires_grad=True, device=dev)
        alpha = (cfg["target_entropy"], log_alpha,
                 make_optim(alpha_kind or optim or v["optim"], [log_alpha], cfg["alpha_lr"],
                            eps))
    policy = DiscreteSACPolicy(nets["actor"], opt["actor"], nets["critic1"], opt["critic1"],
                               nets["critic2"], opt["critic2"], tau=cfg["tau"],
                               gamma=cfg["gamma"], alpha=alpha,
                               estimation_step=v["n_step"]).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy, v


def flat_params(policy):
    """gen_goldens._sac_flat_params on this package's policy, as f64 on the host."""
    mods = [policy.actor, policy.critic1, policy.critic1_old, policy.critic2, policy.critic2_old]
    return np.concatenate([t.detach().cpu().numpy().ravel().astype(np.float64)
                           for m in mods for t in m.parameters()])


def actor_loss_bound(z, tag, u):
    """The actor loss is a signed mean of alpha * H + V: 2e-5 (the critic losses' rtol) of the
    recorded mean magnitudes of its two parts."""
    return 2e-5 * (float(z[tag + "_mag_alpha_h"][u]) + float(z[tag + "_mag_v"][u]))


def alpha_loss_bound(z, cfg, tag, u):
    """alpha_loss = -log_alpha * m with m = mean(target_entropy - H): log_alpha to the
    parameter tolerance (rtol 1e-5 / atol 1e-6), m to 2e-5 of the recorded mean |target_entropy
    - H| (sac_common.alpha_loss_bound's form)."""
    la = float(np.log(np.float64(z[tag + "_alpha_in"][u])))
    t = cfg["target_entropy"] - z[tag + "_ent"][u].astype(np.float64)
    return (1e-6 + 1e-5 * abs(la)) * abs(float(t.mean())) + abs(la) * 2e-5 * float(
        np.abs(t).mean())


# -- the kernels' formulas in f64 NumPy ---------------------------------------------------------------
def row_stats64(logits, q1, q2):
    """(lp, p, H, qm, V) of include/tsrl.h's DiscreteSAC section; NumPy's minimum hands a NaN
    through as torch.min does."""
    l = np.asarray(logits, np.float64)
    m = l.max(axis=1, keepdims=True)
    lp = l - m - np.log(np.exp(l - m).sum(axis=1, keepdims=True))
    p = np.exp(lp)
    H = -np.where(p == 0.0, 0.0, p * lp).sum(axis=1)
    qm = np.minimum(np.asarray(q1, np.float64), np.asarray(q2, np.float64))
    return lp, p, H, qm, (p * qm).sum(axis=1)


def target64(logits, q1, q2, alpha):
    _, _, H, _, V = row_stats64(logits, q1, q2)
    return V + float(alpha) * H


def q_loss64(q1, q2, act, returns, weight):
    """(losses [2], grads [2][b, A], td [b]); f64 throughout (the kernel's td_out is torch's
    f32 expression, checked bitwise elsewhere)."""
    b, A = np.shape(q1)
    w = np.ones(b) if weight is None else np.asarray(weight, np.float64)
    ret = np.asarray(returns, np.float64)
    rows = np.arange(b)
    losses, grads, tds = [], [], []
    for q in (q1, q2):
        td = np.asarray(q, np.float64)[rows, act] - ret
        g = np.zeros((b, A))
        g[rows, act] = 2.0 * td * w / b
        losses.append((td * td * w).mean())
        grads.append(g)
        tds.append(td)
    return np.array(losses), grads, (tds[0] + tds[1]) / 2.0


def actor_loss64(logits, q1, q2, alpha, log_alpha=None, target_entropy=0.0):
    """(loss, g_logits, alpha_loss, g_log_alpha); the last two None without log_alpha."""
    lp, p, H, qm, V = row_stats64(logits, q1, q2)
    b = len(H)
    al = float(alpha)
    loss = -(al * H + V).mean()
    g = -(1.0 / b) * p * ((qm - V[:, None]) - al * (lp + H[:, None]))
    if log_alpha is None:
        return loss, g, None, None
    m = (float(target_entropy) - H).mean()
    return loss, g, -float(log_alpha) * m, -m
