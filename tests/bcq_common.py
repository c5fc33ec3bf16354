"""Shared by tests/test_bcq_host.py and tests/test_gpu_bcq.py: the formulas of
tianshou/policy/imitation/bcq.py and utils/net/continuous.py:371-488 on torch f64 with autograd
-- the judge of csrc/bcq.hip's per-element kernels -- the case list of tsrl_group_linear, and
the policies of tests/golden/bcq.npz (tools/gen_goldens.py gen_bcq: the reference on CPU)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.offline_common import assert_state, state  # noqa: F401  (re-exported)

# (G, R, D, K, H, relu, second output).  G R = 100 on one tile takes the k split; D + K is odd
# in four cases (Wo rows off 16 and 8 bytes); D = 376 with K = 8 is the all-vector path; K = 35
# and D = 1 / 17 end on a half-filled MFMA step; H = 1 / 33 and G = 31 / 33 leave partial tiles.
GROUP_CASES = (
    (1, 100, 17, 6, 256, 1, False), (31, 10, 17, 6, 33, 1, False), (33, 2, 376, 17, 256, 1, True),
    (33, 1, 1, 1, 1, 0, False), (31, 10, 376, 35, 32, 0, False), (1, 2, 1, 35, 32, 0, True),
    (33, 100, 17, 35, 256, 1, False), (31, 2, 376, 6, 1, 0, True), (33, 10, 376, 8, 256, 1, True),
    (10, 100, 376, 17, 256, 1, False))


def vae_case(kind, b, A):
    """Inputs of one VAE case, latent 2 A.  "interior": log_std in [-5, 2] with the lower clamp
    edge below, at and above (-4.5, -4, -3.5) in its first elements; every output is O(1), so a
    bound relative to an output's largest element binds the ordinary elements.  "upper": every
    log_std at 14.5, 15 or 15.5 (std about 3e6) and the noise scaled by 3e-7, so z stays O(1)
    and the elements of each output are again of one magnitude."""
    L = 2 * A
    g = np.random.default_rng(100 * b + A + (kind == "upper"))
    mean, noise = (g.normal(size=(b, L)).astype(np.float32) for _ in range(2))
    if kind == "upper":
        log_std = np.resize(np.float32([15.0, 14.5, 15.5]), (b, L))
        noise *= np.float32(3e-7)
    else:
        log_std = g.uniform(-5, 2, (b, L)).astype(np.float32)
        log_std.flat[:min(3, b * L)] = (-4.0, -4.5, -3.5)[:b * L]
    return dict(mean=mean, log_std=log_std, noise=noise,
                act=g.uniform(-1, 1, (b, A)).astype(np.float32), wd=g.normal(size=(L, A)))


def _leaf(x):
    return torch.as_tensor(x, dtype=torch.float64).requires_grad_()


def vae_ref(mean, log_std, noise, act, wd):
    """continuous.py:461-470 and bcq.py:139-142 with the decoder replaced by recon = z wd:
    (z, std, recon), (vae, recon, KL losses), (g_recon, g_mean, g_log_std)."""
    m, ls = _leaf(mean), _leaf(log_std)
    std = torch.exp(ls.clamp(-4, 15))
    z = m + std * torch.as_tensor(noise, dtype=torch.float64)
    recon = z @ torch.as_tensor(wd, dtype=torch.float64)
    recon.retain_grad()
    rec = F.mse_loss(torch.as_tensor(act, dtype=torch.float64), recon)
    kl = (-torch.log(std) + (std.pow(2) + m.pow(2) - 1) / 2).mean()
    loss = rec + kl / 2
    loss.backward()
    return [t.detach().numpy() for t in (z, std, recon)], \
        np.array([loss.item(), rec.item(), kl.item()]), \
        [t.grad.numpy() for t in (recon, m, ls)]


def perturb_ref(logits, act, phi, m, g_out):
    """continuous.py:405-407: out, g_logits (a [A] logits row is broadcast), g_act."""
    lg, a = _leaf(logits), _leaf(act)
    out = (phi * m * torch.tanh(lg) + a).clamp(-m, m)
    out.backward(torch.as_tensor(g_out, dtype=torch.float64))
    return out.detach().numpy(), lg.grad.numpy(), a.grad.numpy()


def target_ref(q1, q2, rew, done, lmbda, gamma, R):
    """bcq.py:161-172 in f64."""
    q1, q2 = (np.asarray(x, np.float64).reshape(-1, R) for x in (q1, q2))
    v = lmbda * np.minimum(q1, q2) + (1 - lmbda) * np.maximum(q1, q2)
    return rew.astype(np.float64) + (1 - done.astype(np.float64)) * gamma * v.max(1)


# -- the recording ------------------------------------------------------------------------------
def recording(golden_dir):
    z = np.load(os.path.join(golden_dir, "bcq.npz"))
    return z, json.loads(str(z["cfg"]))


def make_policy(z, cfg, tag, dev="cpu", **attrs):
    """The variant's policy over this package's networks, the recorded initial state_dict (the
    reference's checkpoint) loaded with strict=True."""
    from tianshou_amd.policy import BCQPolicy
    from tianshou_amd.utils.net import MLP, VAE, Critic, Net, Perturbation
    v, D, A, H, VH = cfg["variants"][tag], cfg["D"], cfg["A"], cfg["hidden"], cfg["vae_hidden"]
    net_a = MLP(D + A, A, (H, H), device=dev) if v["perturb"] == "mlp" else \
        Net(D + A, A, (H, H), device=dev)
    actor = Perturbation(net_a, max_action=v["max_action"], device=dev, phi=cfg["phi"])
    critics = [Critic(Net(D, A, hidden_sizes=(H, H), concat=True, device=dev), device=dev)
               for _ in range(2)]
    vae = VAE(MLP(D + A, hidden_sizes=(VH, VH), device=dev),
              MLP(D + 2 * A, A, (VH, VH), device=dev), VH, 2 * A, v["max_action"], device=dev)
    nets = [m.to(dev) for m in (actor, *critics, vae)]
    opt = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in nets]
    policy = BCQPolicy(nets[0], opt[0], nets[1], opt[1], nets[2], opt[2], nets[3], opt[3],
                       device=dev, gamma=cfg["gamma"], tau=cfg["tau"], lmbda=cfg["lmbda"],
                       forward_sampled_times=v["T"], num_sampled_action=v["R"])
    policy.load_state_dict(state(z, f"{tag}_init_sd_"), strict=True)
    policy.to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy


def feed_draws(policy, z, tag, updates):
    """Replace the policy's draw hooks by the recorded draws, in the order they were made: the
    updates', then the forward's."""
    def feeder(kind):
        it = (z[f"{tag}_{q}{kind}{i}"] for q in [f"u{u}_" for u in range(updates)] + ["fwd_"]
              for i in range(int(z[f"{tag}_{q}n_{kind}"])))

        def recorded(shape, device="cpu"):
            d = next(it)
            assert tuple(shape) == d.shape, (kind, tuple(shape), d.shape)
            return torch.as_tensor(d, device=device)
        return recorded
    policy._vae_noise, policy._decode_noise = feeder("vae"), feeder("decode")


def check_update(policy, z, tag, u, res, loss_rtol=2e-5):
    """One update's losses (the reference's keys and order: rtol 2e-5 / atol 1e-6) and every
    parameter, online and target (rtol 1e-5 / atol 1e-6)."""
    q = f"{tag}_u{u}_"
    assert list(res) == json.loads(str(z[tag + "_loss_keys"]))
    np.testing.assert_allclose(list(res.values()), z[q + "losses"], rtol=loss_rtol, atol=1e-6,
                               err_msg=q)
    assert_state(policy, z, q + "sd_", q)
