"""Time BCQPolicy.update() (sample + learn) on one filled VectorReplayBuffer and
BCQPolicy.forward(): HIP events around each of --updates calls after --warmup, the legs
interleaved within a run, the whole measurement --runs times.

    python tools/bcq_update_bench.py     # two shapes, three legs x fused_group on / off, 3 runs

Shapes: examples/offline/d4rl_bcq.py's (hidden 256 x 256, VAE 512 x 512, latent 2 A, batch 256,
10 sampled actions per target row) at obs 17 / act 6 and obs 376 / act 17.  ``forward`` acts on
10 observations x 100 samples.
Legs: "graph" (the update replayed from a captured HIP graph), "eager" (the fused kernels and
the flat Adam passes launched eagerly), "torch" (fused=False: the reference's op sequence on the
GPU with optim.step()); the fused legs with ``fused_group`` / ``fused_group_learn`` both on and
both off (off: repeat + cat and the dense first layers; the per-element kernels stay).

Prints one JSON line per (run, shape, leg, fused_group), then per (shape, leg, fused_group) the
median over the runs and the torch leg's spread (max - min of its per-run medians)."""
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
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

from tianshou_amd.data import Batch, VectorReplayBuffer  # noqa: E402
from tianshou_amd.policy import BCQPolicy  # noqa: E402
from tianshou_amd.utils.net import MLP, VAE, Critic, Net, Perturbation  # noqa: E402

dev = torch.device("cuda", 0)
E, T, H, VH, BATCH, ACT_OBS = 8, 512, 256, 512, 256, 10
LEGS = {("graph", True): dict(graph_learn=True), ("graph", False): dict(graph_learn=True),
        ("eager", True): dict(graph_learn=False), ("eager", False): dict(graph_learn=False),
        ("torch", False): dict(fused=False)}


def fill(D, A):
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


def make_policy(D, A, leg, group):
    torch.manual_seed(0)
    actor = Perturbation(MLP(D + A, A, (H, H), device=dev), 1.0, device=dev, phi=0.05).to(dev)
    critics = [Critic(Net(D, A, hidden_sizes=(H, H), concat=True, device=dev), device=dev).to(dev)
               for _ in range(2)]
    vae = VAE(MLP(D + A, hidden_sizes=(VH, VH), device=dev),
              MLP(D + 2 * A, A, (VH, VH), device=dev), VH, 2 * A, 1.0, device=dev).to(dev)
    opt = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in (actor, *critics)] + \
        [torch.optim.Adam(vae.parameters())]
    policy = BCQPolicy(actor, opt[0], critics[0], opt[1], critics[1], opt[2], vae, opt[3],
                       device=dev)
    policy.to(dev)
    policy.train()
    for k, v in dict(LEGS[(leg, group)], fused_group=group, fused_group_learn=group).items():
        setattr(policy, k, v)
    return policy


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


rows = []
for run in range(args.runs):
    for shape in args.shapes.split(","):
        D, A = (int(x) for x in shape.split("x"))
        buf = fill(D, A)
        obs = torch.randn(ACT_OBS, D, device=dev)
        for (leg, group) in LEGS:
            policy = make_policy(D, A, leg, group)
            np.random.seed(0)
            upd, last = timed(lambda: policy.update(BATCH, buf), args.updates)
            assert all(np.isfinite(v) for v in last.values())
            policy.eval()
            with torch.no_grad():
                fwd, act = timed(lambda: policy(Batch(obs=obs, info=Batch())).act, args.updates)
            assert np.shape(act) == (ACT_OBS, A)
            rows.append(dict(run=run, shape=shape, leg=leg, fused_group=group,
                             update_ms_median=round(upd, 4), forward_ms_median=round(fwd, 4),
                             graph_replay=bool(policy._learn_graphs),
                             graph_failed=bool(policy._graph_failed),
                             last_loss=round(float(last["loss/critic1"]), 6)))
            print(json.dumps(rows[-1]), flush=True)

for shape in args.shapes.split(","):
    sel = [r for r in rows if r["shape"] == shape]
    for key in ("update_ms_median", "forward_ms_median"):
        torch_runs = [r[key] for r in sel if r["leg"] == "torch"]
        for (leg, group) in LEGS:
            v = [r[key] for r in sel if r["leg"] == leg and r["fused_group"] == group]
            print(json.dumps(dict(summary=key, shape=shape, leg=leg, fused_group=group,
                                  median_of_runs=round(float(np.median(v)), 4), runs=v,
                                  torch_spread=round(max(torch_runs) - min(torch_runs), 4))))
