"""Time RainbowPolicy.update() (sample + process_fn + learn + post_process_fn, the noise draw
of both networks included) on one filled VectorReplayBuffer: HIP events around each of
--updates updates after --warmup, --runs times over.

    python tools/rainbow_update_bench.py          # two configs, three legs each, three runs

Config "mlp":   Net(12 -> 128 x 3, softmax, 51 atoms) with noisy dueling heads Q (128 -> 128 ->
                6 x 51) and V (128 -> 128 -> 51), batch 64, target network.
Config "atari": net_atari.Rainbow (noisy dueling heads, 51 atoms) on uint8 4 x 84 x 84 frame
                stacks, 6 actions, batch 32, target network.
Legs: "graph" (graph_learn=True: the update replayed from a captured HIP graph whose first node
builds both networks' effective noisy parameters), "eager" (graph_learn=False: the fused kernels
and the flat Adam pass launched eagerly) and "torch" (fused=False: the reference's op sequence
on the GPU, its per-forward weight build included, with optim.step()).

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
ap.add_argument("--configs", default="mlp,atari")
ap.add_argument("--legs", default="graph,eager,torch")
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import RainbowPolicy  # noqa: E402
from tianshou_amd.utils.net import Net, NoisyLinear  # noqa: E402
from tianshou_amd.utils.net_atari import Rainbow  # noqa: E402

dev = torch.device("cuda", 0)
CONFIGS = {
    "mlp": dict(N=51, E=8, T=128, A=6, batch=64, obs=(12,)),
    "atari": dict(N=51, E=8, T=64, A=6, batch=32, obs=(4, 84, 84)),
}
LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


def fill(cfg):
    """Random transitions, episodes ending at 2 % of the steps."""
    E, T, A = cfg["E"], cfg["T"], cfg["A"]
    buf = VectorReplayBuffer(E * T, E, device=dev)
    rng = np.random.default_rng(0)

    def frame():
        if len(cfg["obs"]) == 3:
            return rng.integers(0, 256, (E,) + cfg["obs"], dtype=np.uint8)
        return rng.standard_normal((E,) + cfg["obs"]).astype(np.float32)

    obs = frame()
    for _ in range(T):
        nxt = frame()
        done = rng.random(E) < 0.02
        term = done & (rng.random(E) < 0.5)
        buf.add(Batch(obs=obs, act=rng.integers(0, A, E).astype(np.int64),
                      rew=rng.standard_normal(E), terminated=term, truncated=done & ~term,
                      obs_next=nxt), buffer_ids=np.arange(E))
        obs = nxt
    return buf


def make_policy(cfg, leg):
    torch.manual_seed(0)
    N, A = cfg["N"], cfg["A"]
    if len(cfg["obs"]) == 3:
        net = Rainbow(*cfg["obs"], [A], N, device=dev).to(dev)
        optim = torch.optim.Adam(net.parameters(), lr=1e-4)
        kw = dict(estimation_step=3, target_update_freq=500)
    else:
        head = {"hidden_sizes": (128,), "linear_layer": lambda x, y: NoisyLinear(x, y, 0.5)}
        net = Net(cfg["obs"][0], A, hidden_sizes=(128, 128, 128), device=dev, softmax=True,
                  num_atoms=N, dueling_param=(dict(head), dict(head))).to(dev)
        optim = torch.optim.Adam(net.parameters(), lr=1e-3)
        kw = dict(estimation_step=3, target_update_freq=320)
    policy = RainbowPolicy(net, optim, 0.99, num_atoms=N, **kw).to(dev)
    for k, v in LEGS[leg].items():
        setattr(policy, k, v)
    policy.train()
    return policy


bufs = {name: fill(CONFIGS[name]) for name in args.configs.split(",")}
for run in range(args.runs):
    for name, buf in bufs.items():
        cfg = CONFIGS[name]
        for leg in args.legs.split(","):
            policy = make_policy(cfg, leg)
            np.random.seed(0)
            torch.manual_seed(0)
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
                "obs": list(cfg["obs"]), "atoms": cfg["N"], "updates": args.updates,
                "update_ms_mean": round(float(ms.mean()), 4),
                "update_ms_median": round(float(np.median(ms)), 4),
                "update_ms_min": round(float(ms.min()), 4),
                "update_ms_max": round(float(ms.max()), 4),
                "graph_replay": bool(policy._learn_graphs),
                "flat_optimiser": bool(policy._flat is not None
                                       and policy._flat.adam_bound(policy.optim)),
                "last_loss": round(float(last["loss"]), 6)}), flush=True)
