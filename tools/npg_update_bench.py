"""NPGPolicy / TRPOPolicy.learn: the fused Fisher-vector solve against fused_fvp=False.

Per shape (obs 17 / act 6 and obs 376 / act 17; 1024 and 65536 rows) and policy, one minibatch's
learn is timed three times per leg, the legs alternating in one process on one GPU; medians and
the torch leg's spread (max - min) are printed.  Then tsrl_fvp_apply alone with events at
n = 262144, D = 376, A = 17, next to the time one read of X takes at DESIGN.md's HBM rate.

    python tools/npg_update_bench.py > profiles/npg_update_bench.log
"""
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tianshou-fork_amd")):
    sys.path.insert(0, p)

from tianshou_amd.data import Batch  # noqa: E402
from tianshou_amd.env import Box  # noqa: E402
from tianshou_amd.policy import NPGPolicy, TRPOPolicy  # noqa: E402
from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_actor_critic  # noqa: E402

HBM_TBS = 6.3
dev = torch.device("cuda", 0)


def policy(cls, D, A, fused):
    torch.manual_seed(0)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    actor, critic = actor.to(dev), critic.to(dev)
    init_actor_critic(actor, critic)
    optim = torch.optim.Adam(critic.parameters(), lr=1e-3)
    return cls(actor, critic, optim, fixed_std_normal, action_space=Box(-1.0, 1.0, (A,)),
               fused_fvp=fused).to(dev)


def time_learn(pol, batch, n):
    state = {k: v.clone() for k, v in pol.state_dict().items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pol.learn(batch, n, 1)  # warm-up
        pol.load_state_dict(state)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pol.learn(batch, n, 1)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    print("learn of one minibatch, ms: median of 3 (fused) | median of 3 (torch), torch spread")
    for D, A in ((17, 6), (376, 17)):
        for n in (1024, 65536):
            g = torch.Generator(device=dev).manual_seed(1)
            r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
            batch = Batch(obs=r(n, D), act=r(n, A), adv=r(n), returns=r(n), v_s=r(n),
                          logp_old=-r(n).abs())
            for cls in (NPGPolicy, TRPOPolicy):
                legs = {True: [], False: []}
                for _ in range(3):
                    for fused in (True, False):
                        legs[fused].append(time_learn(policy(cls, D, A, fused), batch, n))
                f, t = statistics.median(legs[True]), statistics.median(legs[False])
                sp = max(legs[False]) - min(legs[False])
                print(f"{cls.__name__} obs {D} act {A} rows {n}: fused {f:.3f} | torch {t:.3f}, "
                      f"spread {sp:.3f} -> {'fused wins' if t - f > sp else 'no win'}")
    n, D, A = 262144, 376, 17
    pol = policy(NPGPolicy, D, A, True)
    obs = torch.randn(n, D, device=dev)
    fvp = pol._fvp_path(Batch(obs=obs))
    fvp.prepare(obs)
    v = torch.randn(fvp.P, device=dev)
    ts = []
    for i in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fvp.apply(v, 0.1)
        e1.record()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append(e0.elapsed_time(e1) * 1e3)
    read = n * ((D + 3) // 4 * 4) * 4 / (HBM_TBS * 1e12) * 1e6
    print(f"tsrl_fvp_apply n {n} D {D} A {A}: median {statistics.median(ts):.1f} us "
          f"(min {min(ts):.1f}); one read of X at {HBM_TBS} TB/s: {read:.1f} us")


if __name__ == "__main__":
    main()
