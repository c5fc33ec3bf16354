"""Time CQLPolicy / TD3BCPolicy.update() (sample + process_fn + learn) on one filled
VectorReplayBuffer: HIP events around each of --updates updates after --warmup, the whole
measurement --runs times.

    python tools/cont_offline_update_bench.py     # two policies, three legs, 3 runs

Shape: the other continuous families' MLP bench (obs 17, 6 actions, 256 x 256 hidden), batch 256,
CQL with 10 repeated actions per row (2560 rows through the logsumexp, 7680 per critic forward),
automatic temperature and the Lagrange multiplier.
Legs: "graph" (graph_learn=True: the update replayed from a captured HIP graph), "eager"
(graph_learn=False: the fused kernels and the flat Adam passes launched eagerly) and "torch"
(fused=False: the reference's op sequence on the GPU with optim.step()).

Prints one JSON line per (run, policy, leg)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="cql,td3bc")
ap.add_argument("--legs", default="graph,eager,torch")
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import CQLPolicy, TD3BCPolicy  # noqa: E402
from tianshou_amd.utils.net import Actor, ActorProb, Critic, Net  # noqa: E402

dev = torch.device("cuda", 0)
E, T, D, A, H, BATCH, R = 8, 512, 17, 6, 256, 256, 10
LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


def fill():
    """Random transitions, episodes ending at 2 % of the steps."""
    buf = VectorReplayBuffer(E * T, E, device=dev)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((E, D)).astype(np.float32)
    for _ in range(T):
        nxt = rng.standard_normal((E, D)).astype(np.float32)
        done = rng.random(E) < 0.02
        term = done & (rng.random(E) < 0.5)
        buf.add(Batch(obs=obs, act=rng.uniform(-1, 1, (E, A)).astype(np.float32),
                      rew=rng.standard_normal(E), terminated=term, truncated=done & ~term,
                      obs_next=nxt), buffer_ids=np.arange(E))
        obs = nxt
    return buf


def make_policy(kind, leg):
    torch.manual_seed(0)
    critics = [Critic(Net(D, A, hidden_sizes=(H, H), concat=True, device=dev), device=dev).to(dev)
               for _ in range(2)]
    if kind == "td3bc":
        actor = Actor(Net(D, hidden_sizes=(H, H), device=dev), (A,), device=dev).to(dev)
    else:
        actor = ActorProb(Net(D, hidden_sizes=(H, H), device=dev), (A,), device=dev,
                          unbounded=True, conditioned_sigma=True).to(dev)
    opt = [torch.optim.Adam(m.parameters(), lr=3e-4) for m in (actor, *critics)]
    nets = (actor, opt[0], critics[0], opt[1], critics[1], opt[2])
    if kind == "td3bc":
        policy = TD3BCPolicy(*nets, exploration_noise=None, action_scaling=False)
    else:
        log_alpha = torch.zeros(1, requires_grad=True, device=dev)
        alpha = (-float(A), log_alpha, torch.optim.Adam([log_alpha], lr=3e-4))
        policy = CQLPolicy(*nets, alpha=alpha, num_repeat_actions=R, device=dev,
                           action_scaling=False)
    policy.to(dev)
    policy.train()
    for k, v in LEGS[leg].items():
        setattr(policy, k, v)
    return policy


for run in range(args.runs):
    buf = fill()
    for kind in args.policies.split(","):
        for leg in args.legs.split(","):
            policy = make_policy(kind, leg)
            np.random.seed(0)
            ms, last = [], None
            for u in range(args.warmup + args.updates):
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                last = policy.update(BATCH, buf)
                t1.record()
                t1.synchronize()
                if u >= args.warmup:
                    ms.append(t0.elapsed_time(t1))
            assert all(np.isfinite(v) for v in last.values())
            ms = np.asarray(ms)
            print(json.dumps({
                "run": run, "policy": kind, "leg": leg, "batch": BATCH, "updates": args.updates,
                "update_ms_mean": round(float(ms.mean()), 4),
                "update_ms_median": round(float(np.median(ms)), 4),
                "update_ms_min": round(float(ms.min()), 4),
                "update_ms_max": round(float(ms.max()), 4),
                "graph_replay": bool(policy._learn_graphs),
                "graph_failed": bool(policy._graph_failed),
                "last_loss": round(float(last["loss/critic1"]), 6)}), flush=True)
