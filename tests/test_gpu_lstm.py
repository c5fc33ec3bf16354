"""csrc/lstm.hip through the C ABI and through Recurrent / RecurrentActorProb / RecurrentCritic,
a DRQN update on a stacked buffer, and the Collector's carried policy state.

Bound (tests/test_gpu_icm.py's): max-abs and 2-norm error against the f64 restatement
(tests/lstm_common.py) at most 4 x the error of the same formulation in f32 on the CPU on identical
inputs, floor 2^-23 of the reference's norm; per parameter block for the gradients.  Every output
sits between NaN guard bands.  Each test prints its measured ratio."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import lstm_common as lc
from tests.icm_common import keep_mask
from tests.test_gpu_icm import _guarded, _intact
from tianshou_amd import _C

pytestmark = pytest.mark.gpu
ENTRY = ("tsrl_lstm_seq_fwd", "tsrl_lstm_seq_bwd")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _table(ts):
    tab = _C.LstmWeights()
    for i, t in enumerate(ts):
        getattr(tab, ("w_ih", "w_hh", "b_ih", "b_hh")[i % 4])[i // 4] = t.data_ptr()
    return tab


def _pitched(t, pad, dev):
    """t on the device as a view whose innermost rows sit ``pad`` floats further apart."""
    if t is None:
        return None
    v = torch.zeros(t.shape[:-1] + (t.shape[-1] + pad,), device=dev)[..., :t.shape[-1]]
    v.copy_(t.float())
    return v


def _run(case, data, dev, want_dx):
    B, T, L, H, Din, _ = case
    params, x, h0, c0, d_out = data
    lib = _C.lib()
    w = [p.float().contiguous().to(dev) for p in params]
    xd, h0d, c0d, dd = _pitched(x, 3, dev), _pitched(h0, 8, dev), _pitched(c0, 8, dev), \
        _pitched(d_out, 4, dev)
    s0 = (h0d.stride(0), h0d.stride(1)) if h0d is not None else (0, 0)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    (hfull, hn), (cfull, cn) = _guarded((B, L, H), dev), _guarded((B, L, H), dev)
    (gfull, grad), (xfull, dx) = _guarded((sum(p.numel() for p in w),), dev), \
        _guarded((B, T, Din), dev)
    nb = int(lib.tsrl_lstm_seq_workspace_bytes(B, T, L, H))
    assert nb == 24 * H * L * T * B
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    head = (xd.data_ptr(), xd.stride(0), xd.stride(1), B, T, Din, L, H, ctypes.byref(_table(w)),
            ptr(h0d), ptr(c0d), *s0)
    _C.check(lib.tsrl_lstm_seq_fwd(*head, hn.data_ptr(), cn.data_ptr(), L * H, H, ws.data_ptr(),
                                   nb, None), "fwd")
    infer = torch.empty_like(hn)  # the inference form: no workspace, same bits
    _C.check(lib.tsrl_lstm_seq_fwd(*head, infer.data_ptr(), None, L * H, H, None, 0, None), "fwd")
    assert torch.equal(infer, hn)
    _C.check(lib.tsrl_lstm_seq_bwd(
        *head, dd.data_ptr(), dd.stride(0), ctypes.byref(_table(lc.split(grad, w))),
        dx.data_ptr() if want_dx else None, T * Din, Din, ws.data_ptr(), nb, None), "bwd")
    assert _intact(hfull, cfull, gfull) and (want_dx or bool(xfull.isnan().all()))
    assert _intact(xfull)
    return hn.cpu(), cn.cpu(), grad.cpu(), dx.cpu()


@pytest.mark.parametrize("case", lc.CASES)
def test_forward_backward_match_f64(dev, case):
    data = lc.make(*case)
    got, again = _run(case, data, dev, True), _run(case, data, dev, False)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], again[:3]))  # same bits, dx or not
    r64, r32 = lc.fwd_bwd(*data), lc.fwd_bwd(*data, torch.float32)
    worst = max(lc.worst_ratio(g, a, b, data[0] if i == 2 else None)
                for i, (g, a, b) in enumerate(zip(got, r32, r64)))
    print(f"lstm_last B,T,L,H,Din,state={case}: worst error ratio to f32 {worst:.3f}")
    assert worst <= 4.0


def test_edges(dev):
    from tianshou_amd.utils.net import Recurrent
    lib, tab = _C.lib(), _C.LstmWeights()
    x = torch.zeros(4, 1, 64, device=dev)
    args = lambda B, H: (x.data_ptr(), 64, 64, B, 1, 64, 1, H, ctypes.byref(tab), None, None, 0, 0)  # noqa: E731
    tail = (None, None, 64, 64, None, 0, None)
    assert lib.tsrl_lstm_seq_fwd(*args(0, 64), *tail) == 0
    assert lib.tsrl_lstm_seq_fwd(*args(4, 64), *tail) == 0  # null outputs: nothing launched
    assert lib.tsrl_lstm_seq_bwd(*args(4, 64), None, 64, None, None, 64, 64, None, 0, None) == 0
    assert lib.tsrl_lstm_seq_fwd(*args(4, 96), *tail) == _C.ERR_LSTM_SHAPE
    assert lib.tsrl_lstm_seq_workspace_bytes(4, 1, 1, 96) == 0
    torch.manual_seed(0)
    net = Recurrent(1, (5,), (3,), dev, hidden_layer_size=96).to(dev)
    obs = torch.randn(7, 2, 5, device=dev)
    out = net(obs)[0]
    net.fused = False
    assert torch.equal(out, net(obs)[0])  # a width the kernels do not take: the torch leg
    net = Recurrent(1, (5,), (3,), dev, hidden_layer_size=64).to(dev)
    net._last(torch.zeros(0, 2, 64, device=dev), None)[0].sum().backward()  # nothing is launched
    assert all(bool((p.grad == 0).all()) for p in net.nn.parameters())


def _net(kind, dev, fused, H=64):
    from tianshou_amd.utils.net import Recurrent, RecurrentActorProb, RecurrentCritic
    torch.manual_seed(2)
    net = {"recurrent": lambda: Recurrent(2, (5,), (3,), dev, H, fused=fused),
           "actor": lambda: RecurrentActorProb(2, (5,), (3,), H, device=dev, fused=fused,
                                               conditioned_sigma=True),
           "critic": lambda: RecurrentCritic(2, (5,), (3,), dev, H, fused=fused)}[kind]()
    return net.to(dev)


def _net_out(kind, net, obs, act, state):
    out = net(obs, act) if kind == "critic" else net(obs, state)[0]
    return torch.cat([o.reshape(-1) for o in (out if isinstance(out, tuple) else (out,))])


@pytest.mark.parametrize("kind", ["recurrent", "actor", "critic"])
def test_nets_fused_match_torch(dev, kind, monkeypatch):
    lib, calls, ws_args = _C.lib(), [], []
    for name in ENTRY:
        monkeypatch.setattr(lib, name, (lambda f, n: lambda *a: (
            calls.append(n), ws_args.append(a[17]) if n == ENTRY[0] else None, f(*a))[2])(
            getattr(lib, name), name))
    g = torch.Generator().manual_seed(1)
    obs, act = torch.randn(37, 3, 5, generator=g), torch.randn(37, 3, generator=g)
    state = dict(hidden=torch.randn(37, 2, 64, generator=g), cell=torch.randn(37, 2, 64, generator=g))
    res = {}
    for leg in (True, False, "f64"):
        net = _net(kind, dev, leg is True)
        d, dt = (torch.device("cpu"), torch.float64) if leg == "f64" else (dev, torch.float32)
        if leg == "f64":  # the torch leg in f64: inputs follow the parameters' dtype
            net = net.cpu().double()
            net.device, net.fused = "cpu", False
        calls.clear()
        args = (kind, net, obs.to(d, dt), act.to(d, dt), {k: v.to(d, dt) for k, v in state.items()})
        out = _net_out(*args)
        if leg is True:  # under no_grad the inference form runs: a null workspace, the same bits
            with torch.no_grad():
                assert torch.equal(_net_out(*args), out)
            assert ws_args[0] is not None and ws_args[1] is None and len(ws_args) == 2
        seed = torch.linspace(-1, 1, out.numel(), dtype=dt, device=d)
        grads = torch.autograd.grad(out, list(net.parameters()), seed, allow_unused=True)
        assert sorted(set(calls)) == (sorted(ENTRY) if leg is True else [])
        res[leg] = (out.detach().cpu(), torch.cat([
            (torch.zeros_like(p) if g is None else g).reshape(-1).cpu()
            for p, g in zip(net.parameters(), grads)]), list(net.parameters()))
    worst = max(lc.worst_ratio(res[True][0], res[False][0], res["f64"][0]),
                lc.worst_ratio(res[True][1], res[False][1], res["f64"][1], res["f64"][2]))
    print(f"{kind}: worst error ratio of the fused leg to the torch leg {worst:.3f}")
    assert worst <= 4.0


def test_drqn_update_fused_matches_torch(dev, monkeypatch):
    """test_drqn.py's shape: Recurrent(layer_num=2), stack_num=4, ignore_obs_next, batch 128."""
    from tianshou_amd.data import Batch, VectorReplayBuffer
    from tianshou_amd.env import Discrete
    from tianshou_amd.policy import DQNPolicy
    from tianshou_amd.utils.net import Recurrent
    E, T, D, A, LR, seen, runs = 8, 40, 4, 2, 1e-3, {}, {}
    rng = np.random.RandomState(5)
    rows = [Batch(obs=rng.randn(E, D).astype(np.float32), act=rng.randint(0, A, E),
                  rew=rng.randn(E), terminated=rng.rand(E) < 0.05, truncated=np.zeros(E, bool),
                  obs_next=rng.randn(E, D).astype(np.float32)) for _ in range(T)]
    learn = DQNPolicy.learn
    monkeypatch.setattr(DQNPolicy, "learn", lambda self, b, **kw: (
        seen.update(obs=b.obs.clone(), act=torch.as_tensor(b.act).clone(),
                    ret=torch.as_tensor(b.returns).clone()), learn(self, b, **kw))[1])
    lib, calls = _C.lib(), []
    for name in ENTRY:
        monkeypatch.setattr(lib, name, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(
            getattr(lib, name), name))
    for fused in (True, False):
        torch.manual_seed(3)
        net = Recurrent(2, (D,), (A,), dev, fused=fused).to(dev)
        init = copy.deepcopy(net)
        policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=LR), 0.9, 3,
                           target_update_freq=10, action_space=Discrete(A)).to(dev)
        buf = VectorReplayBuffer(E * T, E, stack_num=4, ignore_obs_next=True, device=dev)
        for r in rows:
            buf.add(r, buffer_ids=np.arange(E))
        np.random.seed(7)
        policy.train()
        calls.clear()
        res = policy.update(128, buf)
        assert sorted(set(calls)) == (sorted(ENTRY) if fused else [])
        assert seen["obs"].shape == (128, 4, D)
        # neither leg moved the parameters out of the flat optimiser buffer
        flat = policy._flat.flat_param
        assert policy._flat.adam_bound(policy.optim) and all(
            0 <= policy._flat.flat_offset(p) < flat.numel() for p in net.parameters())
        runs[fused] = (res["loss"], torch.cat([p.detach().reshape(-1) for p in
                                               net.parameters()]).cpu())
    # the update in f64 on the CPU from the sampled batch: MSE TD loss, Adam's first step
    p64 = [p.detach().cpu().double().requires_grad_() for p in init.parameters()]
    *lstm, w1, b1, w2, b2 = p64  # parameters(): nn.*, fc1, fc2
    obs, act, ret = (seen[k].cpu() for k in ("obs", "act", "ret"))
    hn, _ = lc.lstm_last(lstm, obs.double() @ w1.T + b1)
    q = (hn[:, -1] @ w2.T + b2)[torch.arange(128), act.long().flatten()]
    loss = (ret.double().flatten() - q).pow(2).mean()
    loss.backward()
    grad = torch.cat([p.grad.reshape(-1) for p in p64])
    torch.optim.Adam(p64, lr=LR).step()
    after = torch.cat([p.detach().reshape(-1) for p in p64])
    keep = keep_mask(init, grad)
    assert float((~keep).double().mean()) <= 0.01
    (lf, pf), (lt, pt) = runs[True], runs[False]
    worst = max(lc.worst_ratio(lf, lt, float(loss.detach())), lc.worst_ratio(pf[keep], pt[keep], after[keep]))
    print(f"DRQN update: worst error ratio of the fused leg to the torch leg {worst:.3f}")
    assert worst <= 4.0


class _Counter(torch.nn.Module):
    """A policy whose state counts its calls per env: state + 1, zeros when None."""

    def __init__(self, kind):
        super().__init__()
        self.kind, self.w = kind, torch.nn.Parameter(torch.zeros(1))

    def forward(self, batch, state=None, **kwargs):
        from tianshou_amd.data import Batch
        n = len(batch.obs)
        if self.kind == "dict":
            old = None if state is None else state["n"]
        else:
            old = state
        new = (torch.zeros(n, 2, device=batch.obs.device) if old is None else old) + 1
        state = {None: None, "tensor": new, "dict": dict(n=new)}[self.kind]
        return Batch(act=torch.tanh(batch.obs[:, :3]), state=state)

    def map_action(self, act):
        return act

    def exploration_noise(self, act, batch):
        return act


@pytest.mark.parametrize("kind", ["tensor", "dict"])
def test_collector_carries_state(dev, kind):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    E, steps, bufs = 6, 11, {}
    for k in (kind, None):
        env = SyntheticVectorEnv(E, (5,), 3, ep_len=4, seed=1, device=dev)
        buf = VectorReplayBuffer(E * steps, E, device=dev)
        coll = Collector(_Counter(k), env, buf)
        coll.collect(n_step=E * 2, random=True)
        assert coll._state is None  # a random step leaves the state alone
        coll.collect(n_step=E * (steps - 2))
        bufs[k] = buf
        if k is None:
            assert coll._state is None
            continue
        state = coll._state if k == "tensor" else coll._state["n"]
        done = buf._meta.done.view(E, steps)[:, 2:].cpu().numpy()
        since = [int(np.argmax(np.r_[d[::-1], True])) for d in done]  # steps after the last done
        assert state[:, 0].cpu().tolist() == since and bool((state[:, 0] == state[:, 1]).all())
        assert 0 in since or min(since) < steps - 2  # some env was reset during the collect
        coll.reset_env()
        assert coll._state is None
    for key in ("obs", "act", "rew", "done"):  # the plumbing changes no bit of the policy's rows
        a, b = (bufs[k]._meta[key][:E * steps].view(E, steps, -1)[:, 2:] for k in (kind, None))
        assert torch.equal(a, b)
