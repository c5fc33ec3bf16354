"""Shared by tests/test_gpu_mlp.py, tests/test_gpu_mlp_bwd.py and tests/test_gpu_mlp_eval.py:
the fragment-layout reader and writer (the latter checked on the host by
tests/test_mlp_layout.py), the perturbed get_actor_critic networks and the torch restatement
of one PPO minibatch (ppo.py:121-142), whole (from the observations) or from the heads' outputs only."""
import torch
from torch.distributions import Independent, Normal


def _rho(r):
    return (r & 3) + 8 * (r >> 2)


def frag_to_rows(frag, n, nt=4):
    """MFMA-fragment layout ([row tile][feature tile][q][lane][4], x6.h frag_off4: lane l's
    16 values as four float4 pieces) -> [n, 32*nt]."""
    ntile = (n + 31) // 32
    f = frag[:ntile * nt * 64 * 16].view(ntile, nt, 4, 64, 4).permute(0, 1, 3, 2, 4)
    f = f.reshape(ntile, nt, 64, 16).cpu()
    out = torch.empty(ntile * 32, nt * 32)
    lane = torch.arange(64)
    for r in range(16):
        feat = _rho(r) + 4 * (lane >> 5)
        rows = lane & 31
        for ft in range(nt):
            out[(torch.arange(ntile)[:, None] * 32 + rows[None, :]).reshape(-1),
                (32 * ft + feat).repeat(ntile)] = f[:, ft, :, r].reshape(-1)
    return out[:n]


def frag_floats(n):
    """tsrl_mlp_frag_floats restated for the CPU (csrc/mlp.hip): whole 128-row blocks of 128
    features."""
    return (n + 127) // 128 * 128 * 128


def rows_to_frag(R, fill=0.0):
    """The inverse of frag_to_rows: [n, 128] -> the frag_floats(n) floats of the x6.h frag_off4
    layout ([row tile][feature tile][q][lane][4]) on R's device; every float of the pad rows
    n.. of the last 128-row block holds fill."""
    n = R.shape[0]
    assert R.dim() == 2 and R.shape[1] == 128 and n > 0
    ntile = frag_floats(n) // (4 * 1024)
    full = torch.full((ntile * 32, 128), fill, dtype=R.dtype, device=R.device)
    full[:n] = R
    lane = torch.arange(64, device=R.device)
    r = torch.arange(16, device=R.device)
    feat = _rho(r)[None, :] + 4 * (lane >> 5)[:, None]          # [64, 16]
    rows = (lane & 31)[:, None].expand(64, 16)
    # [row tile][feature tile][lane][r = 4 q + e] -> [row tile][feature tile][q][lane][e]
    g = full.view(ntile, 32, 4, 32).permute(0, 2, 1, 3)[:, :, rows, feat]
    return g.view(ntile, 4, 64, 4, 4).permute(0, 1, 3, 2, 4).contiguous().view(-1)


def _nets(D, A, dev, seed):
    from tianshou_amd.utils.models import get_actor_critic, init_actor_critic
    torch.manual_seed(seed)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    actor, critic = actor.to(dev), critic.to(dev)
    init_actor_critic(actor, critic)
    with torch.no_grad():
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.add_(0.02 * torch.randn_like(p))
    return actor, critic


def ppo_loss(dist, value, act, logp_old, adv, ret, v_s, kw):
    """ppo.py:121-142 from the policy distribution and the critic's values of the minibatch
    rows: (loss, clip_loss, vf_loss, ent)."""
    if kw.get("norm_adv", True):
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    eps_clip = kw.get("eps_clip", 0.2)
    ratio = (dist.log_prob(act) - logp_old).exp()
    surr1 = ratio * adv
    surr2 = ratio.clamp(1.0 - eps_clip, 1.0 + eps_clip) * adv
    if kw.get("dual_clip"):
        clip1 = torch.min(surr1, surr2)
        clip2 = torch.max(clip1, kw["dual_clip"] * adv)
        clip_loss = -torch.where(adv < 0, clip2, clip1).mean()
    else:
        clip_loss = -torch.min(surr1, surr2).mean()
    if kw.get("value_clip"):
        v_clip = v_s + (value - v_s).clamp(-eps_clip, eps_clip)
        vf_loss = torch.max((ret - value).pow(2), (ret - v_clip).pow(2)).mean()
    else:
        vf_loss = (ret - value).pow(2).mean()
    ent = dist.entropy().mean()
    loss = clip_loss + kw.get("vf_coef", 0.25) * vf_loss - kw.get("ent_coef", 0.01) * ent
    return loss, clip_loss, vf_loss, ent


def gauss_dist(mu, sigma_param):
    """fixed_std_normal on ActorProb's (mu, sigma_param.exp() broadcast to mu); a sigma_param
    already of mu's shape (one copy per row) is taken as it is."""
    if sigma_param.shape != mu.shape:
        sigma_param = sigma_param.view(1, -1) + torch.zeros_like(mu)
    return Independent(Normal(mu, sigma_param.exp()), 1)


def _ref_minibatch(W, obs, act, logp_old, adv, ret, v_s, kw, dtype, device):
    """ppo.py:121-142 on the functional form of get_actor_critic's networks."""
    P = {k: v.detach().to(device, dtype).clone().requires_grad_(True) for k, v in W.items()}
    x = obs.to(device, dtype)
    c = lambda t: t.to(device, dtype)  # noqa: E731
    ha = torch.tanh(torch.tanh(x @ P["w1a"].T + P["b1a"]) @ P["w2a"].T + P["b2a"])
    mu = ha @ P["w3a"].T + P["b3a"]
    hc = torch.tanh(torch.tanh(x @ P["w1c"].T + P["b1c"]) @ P["w2c"].T + P["b2c"])
    value = (hc @ P["w3c"].T + P["b3c"]).flatten()
    loss, clip_loss, vf_loss, ent = ppo_loss(gauss_dist(mu, P["sigma"]), value, c(act),
                                             c(logp_old), c(adv), c(ret), c(v_s), kw)
    loss.backward()
    terms = torch.stack([loss, clip_loss, vf_loss, ent]).detach().cpu().double()
    return terms, {k: v.grad.detach().cpu().double() for k, v in P.items()}
