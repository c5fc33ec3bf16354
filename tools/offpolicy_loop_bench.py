"""Time the whole off-policy loop -- OffpolicyTrainer over a Collector on SyntheticVectorEnv --
for DDPG (update_per_step 1) and REDQ (update_per_step 20, the update-to-data ratio of
examples/mujoco/mujoco_redq.py) on the update benches' shapes: "d17" obs 17 / act 6 and "d376"
obs 376 / act 17, hidden (256, 256), batch 256, n_step 1, the learn step replayed from HIP graphs.
Each (policy, shape) runs once with ``fused_sample`` on (one tsrl_replay_sample launch per
update) and once with it off (the generic sample + compute_nstep_return path).

    python tools/offpolicy_loop_bench.py                       # every leg, a child process each
    python tools/offpolicy_loop_bench.py --policies redq --configs d376 --updates 2000

A leg makes two passes after a warm-up that captures the graphs:
  end-to-end  one trainer epoch; env_steps_per_s from the wall clock around it (one device
              synchronise at each end), update_ms_* from a host clock around every
              policy.update() -- an update ends with the host read of its losses, so the clock
              stops after the device has finished it;
  pre-learn   a second epoch in which update() and learn() each start with a device
              synchronise: pre_learn_ms_* is the host time from the start of update() to the
              start of learn() with the sample's and process_fn's device work complete, and
              pre_learn_share its median over the median of this pass's whole update().  The
              synchronise removes the overlap of host and device, so this pass's figures are
              not comparable with the first pass's.
Prints one JSON line per leg.  Without --leg this process starts every leg as a fresh child
under its own time limit, one after the other, and stops at the first one that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="ddpg,redq")
ap.add_argument("--configs", default="d17,d376")
ap.add_argument("--fused", default="on,off")
ap.add_argument("--updates", type=int, default=1600, help="updates per pass (rounded up to "
                "whole collects)")
ap.add_argument("--warmup-updates", type=int, default=160)
ap.add_argument("--envs", type=int, default=8)
ap.add_argument("--leg-timeout", type=int, default=180, help="seconds per child process")
ap.add_argument("--leg", default=None, help="policy:config:on|off -- run this leg here")
args = ap.parse_args()

if args.leg is None:
    for kind in args.policies.split(","):
        for name in args.configs.split(","):
            for fused in args.fused.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--leg",
                       f"{kind}:{name}:{fused}", "--updates", str(args.updates),
                       "--warmup-updates", str(args.warmup_updates), "--envs", str(args.envs)]
                try:
                    rc = subprocess.run(cmd, timeout=args.leg_timeout).returncode
                except subprocess.TimeoutExpired:
                    raise SystemExit(f"leg {kind}:{name}:{fused} ran into its time limit")
                if rc != 0:  # nothing more is started on the device after a failure
                    raise SystemExit(f"leg {kind}:{name}:{fused} failed with status {rc}")
    raise SystemExit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

from tianshou_amd.data import Collector, VectorReplayBuffer  # noqa: E402
from tianshou_amd.env import SyntheticVectorEnv  # noqa: E402
from tianshou_amd.policy import DDPGPolicy, REDQPolicy  # noqa: E402
from tianshou_amd.trainer import OffpolicyTrainer  # noqa: E402
from tianshou_amd.utils.net import Actor, ActorProb, Critic, EnsembleLinear, Net  # noqa: E402

dev = torch.device("cuda", 0)
CONFIGS = {"d17": dict(D=17, A=6), "d376": dict(D=376, A=17)}
HIDDEN, BATCH, ROWS_PER_ENV = (256, 256), 256, 4096
UPDATE_PER_STEP = {"ddpg": 1, "redq": 20}
REDQ_ENSEMBLE, REDQ_SUBSET = 10, 2


def make_policy(kind, D, A, space):
    torch.manual_seed(0)
    if kind == "ddpg":
        actor = Actor(Net(D, hidden_sizes=HIDDEN, device=dev), (A,), device=dev).to(dev)
        critic = Critic(Net(D, A, hidden_sizes=HIDDEN, concat=True, device=dev),
                        device=dev).to(dev)
        return DDPGPolicy(actor, torch.optim.Adam(actor.parameters(), lr=3e-4), critic,
                          torch.optim.Adam(critic.parameters(), lr=3e-4), tau=0.005, gamma=0.99,
                          exploration_noise=None, estimation_step=1, action_scaling=False,
                          action_space=space).to(dev)
    actor = ActorProb(Net(D, hidden_sizes=HIDDEN, device=dev), (A,), device=dev,
                      unbounded=True, conditioned_sigma=True).to(dev)

    def linear(x, y):
        return EnsembleLinear(REDQ_ENSEMBLE, x, y)

    critics = Critic(Net(D, A, hidden_sizes=HIDDEN, concat=True, device=dev,
                         linear_layer=linear), device=dev, linear_layer=linear,
                     flatten_input=False).to(dev)
    log_alpha = torch.zeros(1, requires_grad=True, device=dev)
    alpha = (-float(A), log_alpha, torch.optim.Adam([log_alpha], lr=3e-4))
    return REDQPolicy(actor, torch.optim.Adam(actor.parameters(), lr=3e-4), critics,
                      torch.optim.Adam(critics.parameters(), lr=3e-4),
                      ensemble_size=REDQ_ENSEMBLE, subset_size=REDQ_SUBSET, tau=0.005,
                      gamma=0.99, alpha=alpha, estimation_step=1, actor_delay=20,
                      action_scaling=False, action_space=space).to(dev)


def stats(prefix, ms):
    ms = np.asarray(ms)
    return {prefix + "_ms_median": round(float(np.median(ms)), 4),
            prefix + "_ms_min": round(float(ms.min()), 4),
            prefix + "_ms_max": round(float(ms.max()), 4)}


def epoch(policy, collector, updates, ups):
    """One trainer epoch of about ``updates`` updates; returns (seconds, env steps)."""
    E = collector.env_num
    steps = -(-updates // (ups * E)) * E
    trainer = OffpolicyTrainer(policy, max_epoch=1, batch_size=BATCH, train_collector=collector,
                               step_per_epoch=steps, step_per_collect=E, update_per_step=ups,
                               episode_per_test=1, show_progress=False, verbose=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in trainer:
        pass
    torch.cuda.synchronize()
    return time.perf_counter() - t0, trainer.env_step, trainer.gradient_step


kind, name, fused = args.leg.split(":")
cfg, ups = CONFIGS[name], UPDATE_PER_STEP[kind]
env = SyntheticVectorEnv(args.envs, (cfg["D"],), cfg["A"], ep_len=1000, device=dev)
policy = make_policy(kind, cfg["D"], cfg["A"], env.action_space)
policy.graph_learn = True
policy.fused_sample = fused == "on"
buf = VectorReplayBuffer(args.envs * ROWS_PER_ENV, args.envs, device=dev)
collector = Collector(policy, env, buf)
np.random.seed(0)
torch.manual_seed(1)
collector.collect(n_step=args.envs * 64)  # something to sample from
epoch(policy, collector, args.warmup_updates, ups)  # graph capture

# pass 1: end to end
update_ms, real_update = [], policy.update


def timed_update(*a, **kw):
    t0 = time.perf_counter()
    res = real_update(*a, **kw)
    update_ms.append((time.perf_counter() - t0) * 1e3)
    return res


policy.update = timed_update
fused_before = buf.fused_samples
seconds, env_steps, n_updates = epoch(policy, collector, args.updates, ups)
fused_taken = buf.fused_samples - fused_before

# pass 2: the part of update() before learn(), device work included
sync_update_ms, pre_ms, real_learn, mark = [], [], policy.learn, [0.0]


def synced_update(*a, **kw):
    torch.cuda.synchronize()
    mark[0] = time.perf_counter()
    res = real_update(*a, **kw)
    sync_update_ms.append((time.perf_counter() - mark[0]) * 1e3)
    return res


def synced_learn(batch, **kw):
    torch.cuda.synchronize()
    pre_ms.append((time.perf_counter() - mark[0]) * 1e3)
    return real_learn(batch, **kw)


policy.update, policy.learn = synced_update, synced_learn
epoch(policy, collector, args.updates, ups)
assert len(pre_ms) == len(sync_update_ms) > 0

print(json.dumps({
    "policy": kind, "config": name, "fused_sample": fused == "on", "batch": BATCH,
    "obs": cfg["D"], "act": cfg["A"], "envs": args.envs, "update_per_step": ups,
    "env_steps": env_steps, "updates": n_updates, "fused_samples": fused_taken,
    "env_steps_per_s": round(env_steps / seconds, 2), **stats("update", update_ms),
    **stats("pre_learn", pre_ms), **stats("synced_update", sync_update_ms),
    "pre_learn_share": round(float(np.median(pre_ms) / np.median(sync_update_ms)), 4),
    "graphs": len(policy._learn_graphs)}), flush=True)
