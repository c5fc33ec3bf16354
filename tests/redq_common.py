"""Shared by tests/test_redq_host.py and tests/test_gpu_redq.py: reading tests/golden/redq.npz
(tools/gen_goldens.py gen_redq) and building the nets, optimisers and policies its variants
name.  Every recorded quantity of a variant is one array, the six updates stacked; what exists
only on updates that step the actor is NaN elsewhere (``did_actor`` says which)."""
import json
import os

import numpy as np
import torch

from tests.ddpg_common import make_optim
from tests.sac_common import alpha_loss_bound, alpha_optim, feed_draws  # noqa: F401

TAGS = ["redq", "redq_auto", "redq_mean", "redq_full", "redq_per", "redq_rms"]
ADAM_TAGS = [t for t in TAGS if t != "redq_rms"]
N_UPDATES = 6
_CACHE = {}


def golden(golden_dir):
    z = _CACHE.get(golden_dir)
    if z is None:
        with np.load(os.path.join(golden_dir, "redq.npz")) as f:
            z = _CACHE[golden_dir] = {k: f[k] for k in f.files}
    return z


def learn_cfg(z):
    return json.loads(str(z["learn_cfg"]))


def make_critics(cfg, dev):
    """The ensemble as examples/mujoco/mujoco_redq.py:92-105 builds it."""
    from tianshou_amd.utils.net import Critic, EnsembleLinear, Net
    D, A, hidden, NE = cfg["D"], cfg["A"], tuple(cfg["hidden"]), cfg["ensemble"]

    def linear(x, y):
        return EnsembleLinear(NE, x, y)

    return Critic(Net(D, A, hidden_sizes=hidden, concat=True, device=dev, linear_layer=linear),
                  device=dev, linear_layer=linear, flatten_input=False).to(dev)


def make_nets(z, cfg, dev):
    """{name: module} with the recorded initial weights."""
    from tianshou_amd.utils.net import ActorProb, Net
    D, A, hidden = cfg["D"], cfg["A"], tuple(cfg["hidden"])
    nets = {"actor": ActorProb(Net(D, hidden_sizes=hidden, device=dev), (A,), device=dev,
                               unbounded=True, conditioned_sigma=True).to(dev),
            "critics": make_critics(cfg, dev)}
    with torch.no_grad():
        for name, net in nets.items():
            for k, p in net.named_parameters():
                p.copy_(torch.as_tensor(z[f"init_{name}.{k}"]))
    return nets


def make_policy(z, cfg, tag, dev, optim=None, alpha_kind=None, **attrs):
    from tianshou_amd.policy import REDQPolicy
    v = cfg["variants"][tag]
    nets = make_nets(z, cfg, dev)
    opt = {n: make_optim(optim or v["optim"], m.parameters()) for n, m in nets.items()}
    alpha = cfg["alpha"]
    if v["auto"]:
        log_alpha = torch.zeros(1, requires_grad=True, device=dev)
        alpha = (cfg["target_entropy"], log_alpha,
                 alpha_optim(alpha_kind or optim or v["optim"], log_alpha, cfg["alpha_lr"]))
    policy = REDQPolicy(nets["actor"], opt["actor"], nets["critics"], opt["critics"],
                        ensemble_size=cfg["ensemble"], subset_size=v["subset"], tau=cfg["tau"],
                        gamma=cfg["gamma"], alpha=alpha, estimation_step=v["n_step"],
                        actor_delay=v["delay"], target_mode=v["mode"],
                        action_scaling=False).to(dev)
    for k, a in attrs.items():
        setattr(policy, k, a)
    return policy, v


def flat_params(policy):
    """gen_goldens._redq_flat_params on this package's policy, as f64 on the host."""
    mods = [policy.actor, policy.critics, policy.critics_old]
    return np.concatenate([t.detach().cpu().numpy().ravel().astype(np.float64)
                           for m in mods for t in m.parameters()])


def did_actor(z, tag, u):
    return bool(z[tag + "_did_actor"][u])


def update_draws(z, tag):
    """The draws of the six recorded updates in the order they were made: one in process_fn,
    one more in learn on the updates that step the actor."""
    out = []
    for u in range(N_UPDATES):
        out.append(z[tag + "_eps_target"][u])
        if did_actor(z, tag, u):
            out.append(z[tag + "_eps_learn"][u])
    return out


def loss_keys(auto, did):
    keys = ("loss/critics",)
    if did:
        keys += ("loss/actor",) + (("loss/alpha", "alpha") if auto else ())
    return keys


def actor_loss_bound(z, tag, u):
    """sac_common.actor_loss_bound with the ensemble mean in place of the min: the actor loss
    is a signed mean of alpha * log_prob - mean_e Q; 2e-5 (the critic loss's rtol) of the mean
    magnitudes of its two parts in the recording."""
    alpha = float(z[tag + "_alpha_in"][u])
    qa = z[tag + "_qa"][u].astype(np.float64).mean(0)
    return 2e-5 * (float(np.abs(alpha * z[tag + "_log_prob"][u]).mean())
                   + float(np.abs(qa).mean()))
