"""The REDQ critic ensemble's forward alone: tsrl_ens_critic_fwd (csrc/ensemble.hip) through
utils.net.ensemble_critic against the torch lines ``critic(obs, act)``, under no_grad, at the
shapes of tools/ddpg_update_bench.py's REDQ legs (10 members, hidden (256, 256), batch 256, obs
17 / act 6 and obs 376 / act 17), all members and a subset of 2.

    python tools/ensemble_kernel_bench.py --iters 500
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/ensemble_kernel_bench.py --iters 50

Per leg: HIP events around --iters back-to-back calls after --warmup (the time of a call in a
saturated queue: kernel plus whatever launch cost the queue does not hide; the kernel alone is
what the kernel trace of the second command shows), three runs, legs alternating.  The bounds
next to them are computed from the shapes: 2 b S (Din H + H H + H) flops at the 157.3 TF/s f32
matrix rate, and one read of the S members' weights, obs and act plus one write of q at 8 TB/s.
--learn adds the training pair at all members: ensemble_critic(learn=True) (tsrl_ens_critic_fwd_save
and one tsrl_ens_critic_bwd) against the torch lines under autograd, forward plus backward, once
towards the six parameters (the critic step, members "w") and once towards the action alone (the
actor step, members "a").  Their bounds: three times the forward's flops for "w" (forward, chain,
weight gradients), twice for "a"; the forward's bytes plus one write and one read of the four
[E, b, H] workspace arrays and, for "w", one write of the gradients.
Prints one JSON line per (shape, members, leg, run)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(os.path.join(ROOT, "tianshou-fork_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--learn", action="store_true", help="add the forward + backward legs")
args = ap.parse_args()

from tianshou_amd.utils.net import Critic, EnsembleLinear, Net, ensemble_critic  # noqa: E402

dev = torch.device("cuda", 0)
E, H, B = 10, 256, 256
MATRIX_FLOPS, HBM_BYTES = 157.3e12, 8.0e12


def timed(fn):
    for _ in range(args.warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / args.iters


for name, D, A in (("d17", 17, 6), ("d376", 376, 17)):
    torch.manual_seed(0)

    def linear(x, y):
        return EnsembleLinear(E, x, y)

    critic = Critic(Net(D, A, hidden_sizes=(H, H), concat=True, device=dev, linear_layer=linear),
                    device=dev, linear_layer=linear, flatten_input=False).to(dev)
    obs, act = torch.randn(B, D, device=dev), torch.randn(B, A, device=dev)
    for members in (None, np.array([7, 2])):
        S = E if members is None else len(members)
        flops = 2.0 * B * S * ((D + A) * H + H * H + H)
        nbytes = 4.0 * (S * ((D + A) * H + H * H + 3 * H + 1) + B * (D + A) + S * B)
        legs = {"kernel": lambda: ensemble_critic(critic, obs, act, members=members),
                "torch": lambda: ensemble_critic(critic, obs, act, members=members, fused=False)}
        with torch.no_grad():
            for run in range(args.runs):
                for leg, fn in legs.items():
                    print(json.dumps({
                        "shape": name, "obs": D, "act": A, "batch": B, "members": S, "leg": leg,
                        "run": run, "call_us": round(timed(fn), 2),
                        "matrix_bound_us": round(flops / MATRIX_FLOPS * 1e6, 3),
                        "hbm_bound_us": round(nbytes / HBM_BYTES * 1e6, 3)}), flush=True)
    if not args.learn:
        continue
    params = list(critic.parameters())
    dq = torch.randn(E, B, 1, device=dev)
    wbytes = 4.0 * E * ((D + A) * H + H * H + 3 * H + 1)
    for tag, mult in (("w", 3.0), ("a", 2.0)):
        a = act.clone().requires_grad_(tag == "a")
        inputs = params if tag == "w" else [a]

        def step(fused, a=a, inputs=inputs, learn=True if tag == "w" else "act"):
            q = ensemble_critic(critic, obs, a, learn=learn) if fused else critic(obs, a)
            torch.autograd.grad(q, inputs, dq)

        flops = mult * 2.0 * B * E * ((D + A) * H + H * H + H)
        nbytes = wbytes * (2 if tag == "w" else 1) + 4.0 * (B * (D + A) + 8 * E * B * H)
        for run in range(args.runs):
            for leg, fn in (("kernel", lambda: step(True)), ("torch", lambda: step(False))):
                print(json.dumps({
                    "shape": name, "obs": D, "act": A, "batch": B, "members": tag,
                    "leg": "learn_" + leg, "run": run, "call_us": round(timed(fn), 2),
                    "matrix_bound_us": round(flops / MATRIX_FLOPS * 1e6, 3),
                    "hbm_bound_us": round(nbytes / HBM_BYTES * 1e6, 3)}), flush=True)
