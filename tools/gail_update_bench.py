"""Time GAILPolicy.update() (process_fn + discriminator steps + PPO epochs) with the fused
discriminator on and off, and process_fn's reward on its own: HIP events around each of
--updates calls after --warmup, the two legs alternating within a run, --runs runs.

    python tools/gail_update_bench.py     # two shapes, fused / torch, 3 runs

Shapes: examples/inverse/irl_gail.py's (obs 17 / act 6, 16 envs x 2048 steps, disc_update_num 2,
10^6 synthetic expert rows, batch 64 -> here 2048 to keep a run short) and obs 376 / act 17 at
4096 envs x 256 steps (disc_update_num 4, 262144 expert rows, batch 262144).

Prints one JSON line per (run, shape, leg), then per (shape, leg) the median over the runs and
the torch leg's spread (max - min of its per-run medians), then the two kernels' bounds from the
shapes: rows x (D + A) x 4 bytes over the HBM bandwidth, and the layer FLOPs over the f32 matrix
peak (compare with a separate ``rocprofv3 --kernel-trace --stats`` run of this tool)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="17x6,376x17")
ap.add_argument("--updates", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--legs", default="fused,torch")
args = ap.parse_args()

from tianshou_amd.data import Batch, ReplayBuffer, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import GAILPolicy  # noqa: E402
from tianshou_amd.utils.models import (  # noqa: E402
    fixed_std_normal, get_actor_critic, init_and_get_optim)
from tianshou_amd.utils.net import Critic, Net  # noqa: E402

dev = torch.device("cuda", 0)
# (envs, steps, disc_update_num, expert rows, PPO batch, repeat)
SHAPES = {"17x6": (16, 2048, 2, 10 ** 6, 2048, 2), "376x17": (4096, 256, 4, 262144, 262144, 2)}
HBM_BYTES_S = 8.0e12      # MI355X: 8 TB/s HBM3E
F32_MATRIX_FLOPS = 157.3e12  # MI355X: f32 matrix peak


def bounds(rows, D, A, step):
    """(HBM-bound us, matrix-bound us) of one launch over ``rows`` rows: the reward reads every
    row once and runs the three layers forward; the step adds the backward chain (dz1, dW1,
    dW2: as many products again, and dW1 a second pass over X from LDS, not HBM)."""
    K = D + A
    fwd = 2.0 * rows * (K * 64 + 64 * 64 + 64)
    flops = fwd + 2.0 * rows * (K * 64 + 2 * 64 * 64 + 64) if step else fwd
    return rows * K * 4 / HBM_BYTES_S * 1e6, flops / F32_MATRIX_FLOPS * 1e6


def fill(D, A, E, T, n_exp):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)  # noqa: E731
    buf = VectorReplayBuffer(E * T, E, device=dev)
    obs = r(E, D)
    for t in range(T):
        nxt = r(E, D)
        done = torch.rand(E, generator=g, device=dev) < 0.02
        buf.add(Batch(obs=obs, act=r(E, A).clamp(-1, 1), rew=torch.zeros(E, device=dev),
                      terminated=done, truncated=torch.zeros_like(done), obs_next=nxt),
                buffer_ids=np.arange(E))
        obs = nxt
    eo, z = r(n_exp, D) + 0.5, torch.zeros(n_exp, device=dev)
    expert = ReplayBuffer(n_exp, device=dev)
    expert.set_batch(Batch(obs=eo, act=r(n_exp, A).clamp(-1, 1), rew=z, terminated=z > 0,
                           truncated=z > 0, done=z > 0, obs_next=eo))
    expert._ring.lengths[0] = n_exp
    return buf, expert


def make_policy(D, A, expert, num, fused):
    torch.manual_seed(0)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    optim = init_and_get_optim(actor, critic, 3e-4)
    disc = Critic(Net((D,), action_shape=(A,), hidden_sizes=(64, 64), activation=torch.nn.Tanh,
                      device=dev, concat=True), device=dev).to(dev)
    disc_optim = torch.optim.Adam(disc.parameters(), lr=2.5e-5)
    return GAILPolicy(actor, critic, optim, fixed_std_normal, expert, disc, disc_optim, num,
                      fused=fused, action_scaling=False, max_grad_norm=0.5, vf_coef=0.25,
                      ent_coef=0.0).to(dev)


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
        D, A = (int(x) for x in shape.split("x"))
        E, T, num, n_exp, bs, rep = SHAPES[shape]
        buf, expert = fill(D, A, E, T, n_exp)
        batch = buf.sample(0)[0]
        for leg in legs:
            policy = make_policy(D, A, expert, num, leg == "fused")
            np.random.seed(0)
            upd, last = timed(lambda: policy.update(0, buf, batch_size=bs, repeat=rep),
                              args.updates)
            assert all(np.isfinite(v).all() for v in last.values())
            rew, _ = timed(lambda: policy.disc_reward(batch), args.updates)
            rows.append(dict(run=run, shape=shape, leg=leg, update_ms_median=round(upd, 4),
                             reward_ms_median=round(rew, 4),
                             last_disc_loss=round(float(last["loss/disc"][-1]), 6)))
            print(json.dumps(rows[-1]), flush=True)
        del buf, expert, batch, policy
        torch.cuda.empty_cache()

for shape in args.shapes.split(","):
    sel = [r for r in rows if r["shape"] == shape]
    for key in ("update_ms_median", "reward_ms_median"):
        torch_runs = [r[key] for r in sel if r["leg"] == "torch"]
        for leg in legs:
            v = [r[key] for r in sel if r["leg"] == leg]
            print(json.dumps(dict(
                summary=key, shape=shape, leg=leg, median_of_runs=round(float(np.median(v)), 4),
                runs=v, torch_spread=round(max(torch_runs) - min(torch_runs), 4)
                if torch_runs else None)))
    D, A = (int(x) for x in shape.split("x"))
    E, T, num = SHAPES[shape][:3]
    n = E * T
    for name, m, step in (("gail_reward_kernel", n, False),
                          ("gail_step_kernel", 2 * (n // num), True)):
        hbm, mat = bounds(m, D, A, step)
        print(json.dumps(dict(bound=name, shape=shape, rows=m, hbm_us=round(hbm, 2),
                              matrix_us=round(mat, 2),
                              bound_by="hbm" if hbm > mat else "matrix")))
