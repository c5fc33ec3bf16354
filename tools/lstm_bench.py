"""Time the recurrent nets' LSTM stack with the fused leg (csrc/lstm.hip) on and off: HIP events
around each of --iters calls after --warmup, the two legs alternating within a run, --runs runs.

    python tools/lstm_bench.py     # four shapes, fused / torch, 3 runs

Shapes (L = 2, H = 128, the reference's test/discrete/test_drqn.py on CartPole: obs 4, 2 actions):
"act16" / "act4096" are Recurrent.forward under no_grad at collection shapes (T = 1, a carried
state, B = 16 / 4096); "fwdbwd" is the stack alone, forward + backward at B = 128, T = 4;
"drqn" is DQNPolicy.update() sampling 128 stacked rows (stack_num 4) of a 20000-row buffer.

Prints one JSON line per (run, shape, leg), then per (shape, leg) the median over the runs and the
torch leg's spread (max - min of its per-run medians)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="act16,act4096,fwdbwd,drqn")
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--legs", default="fused,torch")
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.env import Discrete  # noqa: E402
from tianshou_amd.policy import DQNPolicy  # noqa: E402
from tianshou_amd.utils.net import Recurrent  # noqa: E402

dev = torch.device("cuda", 0)
D, A, L, H = 4, 2, 2, 128


def act_case(B, fused):
    torch.manual_seed(0)
    net = Recurrent(L, (D,), (A,), dev, H, fused=fused).to(dev)
    obs = torch.randn(B, D, device=dev)
    state = dict(hidden=torch.randn(B, L, H, device=dev), cell=torch.randn(B, L, H, device=dev))

    def fn():
        with torch.no_grad():
            return net(obs, state)[0]
    return fn


def fwdbwd_case(fused):
    torch.manual_seed(0)
    net = Recurrent(L, (D,), (A,), dev, H, fused=fused).to(dev)
    x = torch.randn(128, 4, H, device=dev)
    seed = torch.randn(128, H, device=dev)
    params = list(net.nn.parameters())

    def fn():
        return torch.autograd.grad(net._last(x, None)[0], params, seed)[0]
    return fn


def drqn_case(fused, E=10, T=2000):
    torch.manual_seed(0)
    net = Recurrent(L, (D,), (A,), dev, H, fused=fused).to(dev)
    policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), 0.9, 3,
                       target_update_freq=320, action_space=Discrete(A)).to(dev)
    policy.train()
    g = torch.Generator(device=dev).manual_seed(0)
    buf = VectorReplayBuffer(E * T, E, stack_num=4, ignore_obs_next=True, device=dev)
    for _ in range(T):
        done = torch.rand(E, generator=g, device=dev) < 0.02
        buf.add(Batch(obs=torch.randn(E, D, generator=g, device=dev),
                      act=torch.randint(0, A, (E,), generator=g, device=dev),
                      rew=torch.ones(E, device=dev), terminated=done,
                      truncated=torch.zeros_like(done),
                      obs_next=torch.randn(E, D, generator=g, device=dev)),
                buffer_ids=np.arange(E))
    np.random.seed(0)
    return lambda: policy.update(128, buf)["loss"]


CASES = {"act16": lambda f: act_case(16, f), "act4096": lambda f: act_case(4096, f),
         "fwdbwd": fwdbwd_case, "drqn": drqn_case}


def timed(fn, n):
    ms = []
    for u in range(args.warmup + n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if u >= args.warmup:
            ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


legs, rows = args.legs.split(","), []
for run in range(args.runs):
    for shape in args.shapes.split(","):
        for leg in legs:
            rows.append(dict(run=run, shape=shape, leg=leg,
                             ms_median=round(timed(CASES[shape](leg == "fused"), args.iters), 4)))
            print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()

for shape in args.shapes.split(","):
    sel = [r for r in rows if r["shape"] == shape]
    torch_runs = [r["ms_median"] for r in sel if r["leg"] == "torch"]
    for leg in legs:
        v = [r["ms_median"] for r in sel if r["leg"] == leg]
        print(json.dumps(dict(
            summary="ms_median", shape=shape, leg=leg, median_of_runs=round(float(np.median(v)), 4),
            runs=v, torch_spread=round(max(torch_runs) - min(torch_runs), 4) if torch_runs else None)))
