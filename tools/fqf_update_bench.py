"""Time FQFPolicy.update() (sample + process_fn + learn + post_process_fn) on one filled
VectorReplayBuffer: HIP events around each of --updates updates after --warmup, the whole
measurement --repeats times per (config, leg).

    python tools/fqf_update_bench.py          # two configs, three legs each, three runs

Config "fqf_mlp":   FullQuantileFunction(Net(12 -> 64 x 2 -> 64), 64 x 3 head, 64 cosines) and
                    FractionProposalNetwork(32, 64) (test/discrete/test_fqf.py's networks), batch
                    64, 32 fractions, ent_coef 10, target network.
Config "fqf_atari": FullQuantileFunction(net_atari.DQN(features_only=True), hidden 512, 64
                    cosines) on uint8 4 x 84 x 84 frame stacks, 6 actions, batch 32, 32 fractions
                    (examples/atari/atari_fqf.py).
Legs: "graph" (graph_learn=True: the update replayed from a captured HIP graph), "eager"
(graph_learn=False: the fused kernels and the flat Adam pass launched eagerly) and "torch"
(fused=False: the reference's op sequence on the GPU with optim.step()).

Prints one JSON line per (config, leg, run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="fqf_mlp,fqf_atari")
ap.add_argument("--legs", default="graph,eager,torch")
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import FQFPolicy  # noqa: E402
from tianshou_amd.utils.net import FractionProposalNetwork, FullQuantileFunction, Net  # noqa: E402
from tianshou_amd.utils.net_atari import DQN  # noqa: E402

dev = torch.device("cuda", 0)
CONFIGS = {
    "fqf_mlp": dict(E=8, T=128, A=6, batch=64, obs=(12,)),
    "fqf_atari": dict(E=8, T=64, A=6, batch=32, obs=(4, 84, 84)),
}
LEGS = {"graph": dict(fused=True, graph_learn=True), "eager": dict(fused=True, graph_learn=False),
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
    A = cfg["A"]
    if len(cfg["obs"]) == 3:
        feature = DQN(*cfg["obs"], [A], device=dev, features_only=True)
        net = FullQuantileFunction(feature, [A], hidden_sizes=[512], num_cosines=64,
                                   device=dev).to(dev)
        optim = torch.optim.Adam(net.parameters(), lr=5e-5)
        kw = dict(estimation_step=3, target_update_freq=500)
    else:
        feature = Net(cfg["obs"][0], 64, hidden_sizes=[64, 64], device=dev)
        net = FullQuantileFunction(feature, [A], hidden_sizes=[64, 64, 64], num_cosines=64,
                                   device=dev).to(dev)
        optim = torch.optim.Adam(net.parameters(), lr=3e-3)
        kw = dict(estimation_step=3, target_update_freq=320)
    propose = FractionProposalNetwork(32, net.input_dim).to(dev)
    frac_optim = torch.optim.RMSprop(propose.parameters(), lr=2.5e-9)
    policy = FQFPolicy(net, optim, propose, frac_optim, 0.99, num_fractions=32, ent_coef=10.0,
                       **kw).to(dev)
    for k, v in LEGS[leg].items():
        setattr(policy, k, v)
    policy.train()
    return policy


for name in args.configs.split(","):
    cfg = CONFIGS[name]
    buf = fill(cfg)
    for run in range(args.repeats):
        for leg in args.legs.split(","):
            policy = make_policy(cfg, leg)
            np.random.seed(0)
            ms, last = [], None
            for u in range(args.warmup + args.updates):
                t0, t1 = torch.cuda.Event(enable_timing=True), \
                    torch.cuda.Event(enable_timing=True)
                t0.record()
                last = policy.update(cfg["batch"], buf)
                t1.record()
                t1.synchronize()
                if u >= args.warmup:
                    ms.append(t0.elapsed_time(t1))
            assert np.isfinite(last["loss"])
            ms = np.asarray(ms)
            print(json.dumps({
                "config": name, "leg": leg, "run": run, "batch": cfg["batch"],
                "obs": list(cfg["obs"]), "fractions": 32, "updates": args.updates,
                "update_ms_mean": round(float(ms.mean()), 4),
                "update_ms_median": round(float(np.median(ms)), 4),
                "update_ms_min": round(float(ms.min()), 4),
                "update_ms_max": round(float(ms.max()), 4),
                "graph_replay": bool(policy._learn_graphs),
                "flat_optimiser": bool(policy._flat is not None
                                       and policy._flat.adam_bound(policy.optim)
                                       and policy._frac_flat is not None
                                       and policy._frac_flat.adam_bound(policy._fraction_optim)),
                "last_loss": round(float(last["loss"]), 6)}), flush=True)
