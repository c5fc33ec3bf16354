"""Time BranchingDQNPolicy.update() (sample + process_fn + learn + post_process_fn) on one
filled VectorReplayBuffer: HIP events around each of --updates updates after --warmup, the
whole measurement --runs times.

    python tools/bdq_update_bench.py              # both configs, three legs, three runs

The two shapes are the reference's own scripts':
Config "pendulum" (test/discrete/test_bdq.py): obs 3, K 1, A 40, hidden 64/64 | 64 | 64,
batch 128.
Config "bipedal" (examples/box2d/bipedal_bdq.py): obs 24, K 4, A 25, hidden 512/256 | 128 |
128, batch 512.
Legs: "graph" (graph_learn=True: the update replayed from a captured HIP graph), "eager"
(graph_learn=False: the fused kernels and the flat Adam pass launched eagerly) and "torch"
(fused=False with BranchingNet.fused_combine=False: the reference's op sequence on the GPU
with optim.step()).

Prints one JSON line per (run, config, leg)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="pendulum,bipedal")
ap.add_argument("--legs", default="graph,eager,torch")
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import BranchingDQNPolicy  # noqa: E402
from tianshou_amd.utils.net import BranchingNet  # noqa: E402

dev = torch.device("cuda", 0)
CONFIGS = {
    "pendulum": dict(E=8, T=128, obs=3, K=1, A=40, common=[64, 64], value=[64], action=[64],
                     batch=128, freq=200, lr=1e-3),
    "bipedal": dict(E=8, T=256, obs=24, K=4, A=25, common=[512, 256], value=[128],
                    action=[128], batch=512, freq=1000, lr=1e-4),
}
LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


def fill(cfg):
    """Random transitions, episodes ending at 2 % of the steps."""
    E, T, K, A = cfg["E"], cfg["T"], cfg["K"], cfg["A"]
    buf = VectorReplayBuffer(E * T, E, device=dev)
    rng = np.random.default_rng(0)
    obs = rng.standard_normal((E, cfg["obs"])).astype(np.float32)
    for _ in range(T):
        nxt = rng.standard_normal((E, cfg["obs"])).astype(np.float32)
        done = rng.random(E) < 0.02
        term = done & (rng.random(E) < 0.5)
        buf.add(Batch(obs=obs, act=rng.integers(0, A, (E, K)).astype(np.int64),
                      rew=rng.standard_normal(E), terminated=term, truncated=done & ~term,
                      obs_next=nxt), buffer_ids=np.arange(E))
        obs = nxt
    return buf


def make_policy(cfg, leg):
    torch.manual_seed(0)
    net = BranchingNet(cfg["obs"], cfg["K"], cfg["A"], cfg["common"], cfg["value"],
                       cfg["action"], device=dev).to(dev)
    optim = torch.optim.Adam(net.parameters(), lr=cfg["lr"])
    policy = BranchingDQNPolicy(net, optim, discount_factor=0.99,
                                target_update_freq=cfg["freq"]).to(dev)
    for k, v in LEGS[leg].items():
        setattr(policy, k, v)
    if leg == "torch":
        policy.model.fused_combine = policy.model_old.fused_combine = False
    return policy


for run in range(args.runs):
    for name in args.configs.split(","):
        cfg = CONFIGS[name]
        buf = fill(cfg)
        for leg in args.legs.split(","):
            policy = make_policy(cfg, leg)
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
            print(json.dumps({
                "run": run, "config": name, "leg": leg, "batch": cfg["batch"],
                "obs": cfg["obs"], "K": cfg["K"], "A": cfg["A"],
                "param_tensors": len(list(policy.model.parameters())),
                "updates": args.updates, "update_ms_mean": round(float(ms.mean()), 4),
                "update_ms_median": round(float(np.median(ms)), 4),
                "update_ms_min": round(float(ms.min()), 4),
                "update_ms_max": round(float(ms.max()), 4),
                "graph_replay": bool(policy._learn_graphs),
                "flat_optimiser": bool(policy._flat is not None
                                       and policy._flat.adam_bound(policy.optim)),
                "last_loss": round(float(last["loss"]), 6)}), flush=True)
