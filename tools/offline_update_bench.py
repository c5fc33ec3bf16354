"""Time DiscreteBCQPolicy / DiscreteCQLPolicy / DiscreteCRRPolicy.update() (sample + process_fn +
learn) on one filled VectorReplayBuffer: HIP events around each of --updates updates after
--warmup, the whole measurement --runs times.

    python tools/offline_update_bench.py          # three policies, two shapes, three legs, 3 runs

Shape "mlp": the recorded shape of tests/golden/offline.npz scaled to the other families' bench
(obs 12 -> 128 x 3 trunk, heads of 128, 6 actions, 51 quantiles for CQL), batch 64.
Shape "atari": uint8 4 x 84 x 84 frame stacks, net_atari.DQN(features_only=True) as the trunk
that BCQ's model and imitator and CRR's actor and critic SHARE (examples/offline/atari_bcq.py,
atari_crr.py), heads of 512, net_atari.QRDQN with 200 quantiles for CQL (atari_cql.py), 6
actions, batch 32.
Legs: "graph" (graph_learn=True: the update replayed from a captured HIP graph), "eager"
(graph_learn=False: the fused kernels and the flat Adam pass launched eagerly) and "torch"
(fused=False: the reference's op sequence on the GPU with optim.step()).

Prints one JSON line per (run, policy, shape, leg)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--policies", default="bcq,cql,crr")
ap.add_argument("--shapes", default="mlp,atari")
ap.add_argument("--legs", default="graph,eager,torch")
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import (DiscreteBCQPolicy, DiscreteCQLPolicy,  # noqa: E402
                                 DiscreteCRRPolicy)
from tianshou_amd.utils.net import DiscreteActor, DiscreteCritic, Net  # noqa: E402
from tianshou_amd.utils.net_atari import DQN, QRDQN  # noqa: E402

dev = torch.device("cuda", 0)
A = 6
SHAPES = {"mlp": dict(E=8, T=128, obs=(12,), batch=64, N=51, head=128),
          "atari": dict(E=8, T=64, obs=(4, 84, 84), batch=32, N=200, head=512)}
LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


def fill(cfg):
    """Random transitions, episodes ending at 2 % of the steps."""
    E, T = cfg["E"], cfg["T"]
    buf = VectorReplayBuffer(E * T, E, device=dev)
    rng = np.random.default_rng(0)

    def draw():
        if len(cfg["obs"]) == 3:
            return rng.integers(0, 256, (E,) + cfg["obs"], dtype=np.uint8)
        return rng.standard_normal((E,) + cfg["obs"]).astype(np.float32)

    obs = draw()
    for _ in range(T):
        nxt = draw()
        done = rng.random(E) < 0.02
        term = done & (rng.random(E) < 0.5)
        buf.add(Batch(obs=obs, act=rng.integers(0, A, E).astype(np.int64),
                      rew=rng.standard_normal(E), terminated=term, truncated=done & ~term,
                      obs_next=nxt), buffer_ids=np.arange(E))
        obs = nxt
    return buf


def make_policy(kind, shape, cfg, leg):
    torch.manual_seed(0)
    atari, H = shape == "atari", cfg["head"]
    if kind == "cql":
        nets = [QRDQN(*cfg["obs"], [A], cfg["N"], device=dev) if atari else
                Net(cfg["obs"], A, hidden_sizes=(H, H, H), num_atoms=cfg["N"], device=dev)]
    else:  # one trunk under both heads
        trunk = DQN(*cfg["obs"], [A], device=dev, features_only=True) if atari else \
            Net(cfg["obs"], hidden_sizes=(H, H, H), device=dev)
        second = DiscreteCritic(trunk, hidden_sizes=[H], last_size=A, device=dev) \
            if kind == "crr" else \
            DiscreteActor(trunk, [A], hidden_sizes=[H], softmax_output=False, device=dev)
        nets = [DiscreteActor(trunk, [A], hidden_sizes=[H], softmax_output=False, device=dev),
                second]
    for n in nets:
        n.to(dev)
    params = list({id(p): p for n in nets for p in n.parameters()}.values())
    optim = torch.optim.Adam(params, lr=1e-4)
    if kind == "bcq":
        policy = DiscreteBCQPolicy(nets[0], nets[1], optim, 0.99, 1, 500)
    elif kind == "cql":
        policy = DiscreteCQLPolicy(nets[0], optim, 0.99, cfg["N"], 1, 500, min_q_weight=10.0)
    else:
        policy = DiscreteCRRPolicy(nets[0], nets[1], optim, 0.99, target_update_freq=500,
                                   action_scaling=False)
    policy.to(dev)
    for k, v in LEGS[leg].items():
        setattr(policy, k, v)
    return policy


for run in range(args.runs):
    for shape in args.shapes.split(","):
        cfg = SHAPES[shape]
        buf = fill(cfg)
        for kind in args.policies.split(","):
            for leg in args.legs.split(","):
                policy = make_policy(kind, shape, cfg, leg)
                np.random.seed(0)
                ms, last = [], None
                for u in range(args.warmup + args.updates):
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    last = policy.update(cfg["batch"], buf)
                    t1.record()
                    t1.synchronize()
                    if u >= args.warmup:
                        ms.append(t0.elapsed_time(t1))
                assert np.isfinite(last["loss"])
                ms = np.asarray(ms)
                flat = getattr(policy, "_flat", None)
                print(json.dumps({
                    "run": run, "policy": kind, "shape": shape, "leg": leg,
                    "batch": cfg["batch"], "updates": args.updates,
                    "update_ms_mean": round(float(ms.mean()), 4),
                    "update_ms_median": round(float(np.median(ms)), 4),
                    "update_ms_min": round(float(ms.min()), 4),
                    "update_ms_max": round(float(ms.max()), 4),
                    "graph_replay": bool(policy._learn_graphs),
                    "graph_failed": bool(policy._graph_failed),
                    "flat_optimiser": bool(flat is not None and flat.adam_bound(policy.optim)),
                    "last_loss": round(float(last["loss"]), 6)}), flush=True)
