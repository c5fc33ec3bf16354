"""Time ICMPolicy.update() (process_fn + the inner policy's learn + the curiosity step) with the
fused head on and off: HIP events around each of --updates calls after --warmup, the two legs
alternating within a run, --runs runs.

    python tools/icm_update_bench.py     # two shapes, fused / torch, 3 runs

Shapes (the reference's test/modelbased/test_dqn_icm.py and test_ppo_icm.py: CartPole, obs 4, 2
actions, inner hidden [128] * 4, feature net MLP(4 -> 128 -> 128), curiosity hidden [128]): "dqn"
samples 64 rows of a 20000-row buffer per update, "ppo" takes all 2048 rows of a 16-env x
128-step rollout (batch 64 -> here 512, repeat 2, to keep a run short).

Prints one JSON line per (run, shape, leg), then per (shape, leg) the median over the runs and
the torch leg's spread (max - min of its per-run medians), then the step kernel's matrix bound
from the shapes: the head's FLOPs over the f32 matrix peak (compare with a separate
``rocprofv3 --kernel-trace --stats`` run of this tool; the weights, 260 KB, stay in L2, so HBM
traffic is the rows only and never binds)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="dqn,ppo")
ap.add_argument("--updates", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--legs", default="fused,torch")
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.env import Discrete  # noqa: E402
from tianshou_amd.policy import DQNPolicy, ICMPolicy, PPOPolicy  # noqa: E402
from tianshou_amd.utils.net import (  # noqa: E402
    MLP, ActorCritic, DiscreteActor, DiscreteCritic, IntrinsicCuriosityModule, Net)

dev = torch.device("cuda", 0)
D, A, W, HID = 4, 2, 128, (128, 128, 128, 128)
# (envs, steps, rows sampled per update (0: all), update kwargs)
SHAPES = {"dqn": (10, 2000, 64, {}), "ppo": (16, 128, 0, dict(batch_size=512, repeat=2))}
F32_MATRIX_FLOPS = 157.3e12  # MI355X: f32 matrix peak


def fill(E, T):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    buf = VectorReplayBuffer(E * T, E, device=dev)
    obs = r(E, D)
    for t in range(T):
        nxt = r(E, D)
        done = torch.rand(E, generator=g, device=dev) < 0.02
        buf.add(Batch(obs=obs, act=torch.randint(0, A, (E,), generator=g, device=dev),
                      rew=torch.ones(E, device=dev), terminated=done,
                      truncated=torch.zeros_like(done), obs_next=nxt), buffer_ids=np.arange(E))
        obs = nxt
    return buf


def make_policy(shape, fused):
    torch.manual_seed(0)
    if shape == "dqn":
        net = Net(D, A, hidden_sizes=HID, device=dev).to(dev)
        inner = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), 0.9, 3,
                          target_update_freq=320, action_space=Discrete(A)).to(dev)
    else:
        actor = DiscreteActor(Net(D, hidden_sizes=HID, device=dev), A, softmax_output=False,
                              device=dev).to(dev)
        critic = DiscreteCritic(Net(D, hidden_sizes=HID, device=dev), device=dev).to(dev)
        optim = torch.optim.Adam(ActorCritic(actor, critic).parameters(), lr=3e-4)
        inner = PPOPolicy(actor, critic, optim,
                          lambda q: torch.distributions.Categorical(logits=q),
                          action_space=Discrete(A), max_grad_norm=0.5, vf_coef=0.5,
                          ent_coef=0.0, action_scaling=False).to(dev)
    model = IntrinsicCuriosityModule(MLP(D, output_dim=W, hidden_sizes=(W,), device=dev), W, A,
                                     hidden_sizes=(W,), device=dev).to(dev)
    return ICMPolicy(inner, model, torch.optim.Adam(model.parameters(), lr=1e-3), lr_scale=1.0,
                     reward_scale=0.01, forward_loss_weight=0.2, fused=fused).to(dev)


def timed(fn, n):
    ms = []
    for u in range(args.warmup + n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        t1.synchronize()
        if u >= args.warmup:
            ms.append(t0.elapsed_time(t1))
    return float(np.median(ms)), out


legs = args.legs.split(",")
rows = []
for run in range(args.runs):
    for shape in args.shapes.split(","):
        E, T, sample, kw = SHAPES[shape]
        buf = fill(E, T)
        for leg in legs:
            policy = make_policy(shape, leg == "fused")
            assert (policy._head is not None) and policy.fused == (leg == "fused")
            np.random.seed(0)
            upd, last = timed(lambda: policy.update(sample, buf, **kw), args.updates)
            assert all(np.isfinite(v).all() for v in last.values())
            rows.append(dict(run=run, shape=shape, leg=leg, update_ms_median=round(upd, 4),
                             last_icm_loss=round(float(last["loss/icm"]), 6)))
            print(json.dumps(rows[-1]), flush=True)
        del buf, policy
        torch.cuda.empty_cache()

for shape in args.shapes.split(","):
    sel = [r for r in rows if r["shape"] == shape]
    torch_runs = [r["update_ms_median"] for r in sel if r["leg"] == "torch"]
    for leg in legs:
        v = [r["update_ms_median"] for r in sel if r["leg"] == leg]
        print(json.dumps(dict(
            summary="update_ms_median", shape=shape, leg=leg,
            median_of_runs=round(float(np.median(v)), 4), runs=v,
            torch_spread=round(max(torch_runs) - min(torch_runs), 4) if torch_runs else None)))
    E, T, sample, _ = SHAPES[shape]
    m = sample or E * T
    # forward 2 M (W (W + 1) + W W + 2 W W + W A), backward twice that (dX and dW products)
    flops = 3 * 2.0 * m * (W * (W + 1) + W * W + 2 * W * W + W * A)
    print(json.dumps(dict(bound="icm_kernel<128, true>", shape=shape, rows=m,
                          matrix_us=round(flops / F32_MATRIX_FLOPS * 1e6, 3),
                          tiles=(m + 31) // 32, bound_by="matrix")))
