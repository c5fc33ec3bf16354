"""tests/golden/dist_dqn.npz (tools/gen_goldens.py gen_dist_dqn: the reference C51Policy and
QRDQNPolicy on CPU torch) pinned on the host: a torch-CPU restatement of c51.py:65-108 and
qrdqn.py:58-97 replays every variant from the recorded sample indices (and, for the prioritized
variants, the recorded importance weights).  tests/test_gpu_dist_dqn.py compares the device
policies with the same file.

Tolerances: n-step returns exact in f32 (the same CPU torch forwards feed the f64 n-step
oracle, oracle/ref.py nstep_return); losses, outgoing weights and parameters rtol 1e-6
(autograd's own kernels against the reference's: same library, possibly another summation
split), as tests/test_dqn_host.py."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref
from tests import test_dqn_host as dh
from tests.conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "dist_dqn.npz"))


def make_net(z, cfg, kind, n_atoms):
    sizes = [cfg["D"], *cfg["hidden"], cfg["A"] * n_atoms]
    layers = []
    for i in range(len(sizes) - 1):
        layers += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    net = torch.nn.Sequential(*layers[:-1])
    dh.load(net, z, f"init_{kind}_")
    return net


def dist(net, x, kind, A, N):
    """[b, A, N]: probabilities (C51) or quantile values (QR-DQN)."""
    y = net(x).view(len(x), A, N)
    return torch.softmax(y, dim=-1) if kind == "c51" else y


def q_values(d, kind, support):
    return (d * support).sum(2) if kind == "c51" else d.mean(2)


def top2_gap(q):
    q = np.sort(np.asarray(q, np.float64), axis=1)
    best, second = q[:, -1], q[:, -2]
    return float(((best - second) / np.maximum(np.abs(best), np.abs(second))).min())


def select_next(net, old, s_next, kind, A, N, support, gaps):
    """c51.py:74-81 / qrdqn.py:60-68: the target network's atoms of the online network's
    greedy action."""
    with torch.no_grad():
        d_new = dist(net, s_next, kind, A, N)
        d_old = dist(old, s_next, kind, A, N)
        q64 = q_values(d_new.double(), kind, None if support is None else support.double())
        gaps.append(top2_gap(q64.numpy()))
        act = q_values(d_new, kind, support).max(dim=1)[1]
        return d_old[np.arange(len(act)), act, :]


def test_variants_replay_from_recorded_indices(z):
    cfg = json.loads(str(z["learn_cfg"]))
    vb, store = dh.host_buffer(z, cfg)
    np.testing.assert_array_equal(vb.sizes, z["buf_lengths"])
    np.testing.assert_array_equal(vb.last_index, z["buf_last_index"])
    A = cfg["A"]
    assert set(cfg["variants"]) == {"c51_target", "c51_notarget", "c51_per", "qr_target",
                                    "qr_notarget", "qr_per", "qr_rms"}
    clamped = {"low": False, "high": False}
    for tag, v in cfg["variants"].items():
        kind = v["kind"]
        N = cfg["c51"]["num_atoms"] if kind == "c51" else cfg["qr"]["num_quantiles"]
        net = make_net(z, cfg, kind, N)
        old = make_net(z, cfg, kind, N) if v["freq"] > 0 else net
        if v["optim"] == "rms":
            optim = torch.optim.RMSprop(net.parameters(), lr=7e-4, eps=1e-5, alpha=0.99)
        else:
            optim = torch.optim.Adam(net.parameters(), lr=1e-3)
        support = tau_hat = None
        if kind == "c51":
            v_min, v_max = cfg["c51"]["v_min"], cfg["c51"]["v_max"]
            support = torch.linspace(v_min, v_max, N)
            delta_z = (v_max - v_min) / (N - 1)
        else:
            tau = torch.linspace(0, 1, N + 1)
            tau_hat = ((tau[:-1] + tau[1:]) / 2).view(1, -1, 1)
        gaps = []
        for u in range(6):
            q = f"{tag}_u{u}_"
            idx = z[q + "indices"]
            assert len(idx) == v["bs"]
            terminal = idx % vb.maxsize
            for _ in range(v["n_step"] - 1):
                terminal = vb.next(terminal)
            # process_fn: _target_q at the chain's last row, then the n-step return
            if kind == "c51":
                tq = support.repeat(len(idx), 1)
            else:
                tq = select_next(net, old, torch.as_tensor(store["obs_next"][terminal]), kind,
                                 A, N, None, gaps)
            returns, _ = ref.nstep_return(vb, store["terminated"], idx, tq.numpy(),
                                          cfg["gamma"], v["n_step"])
            assert returns.dtype == np.float32 and returns.shape == (v["bs"], N)
            np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
            ret = torch.as_tensor(returns)
            # learn
            if v["freq"] > 0 and u % v["freq"] == 0:
                old.load_state_dict(net.state_dict())
            optim.zero_grad()
            w = torch.as_tensor(z[q + "weight"]) if v.get("per") else 1.0
            rows = np.arange(len(idx))
            if kind == "c51":
                # c51.py:73-89 acts on batch.obs_next (the sampled row's own successor)
                next_dist = select_next(net, old, torch.as_tensor(store["obs_next"][idx]), kind,
                                        A, N, support, gaps)
                clamped["low"] |= bool((ret < v_min).any())
                clamped["high"] |= bool((ret > v_max).any())
                tz = ret.clamp(v_min, v_max)
                target = ((1 - (tz.unsqueeze(1) - support.view(1, -1, 1)).abs() / delta_z)
                          .clamp(0, 1) * next_dist.unsqueeze(1)).sum(-1)
                np.testing.assert_allclose(target.numpy(), z[q + "target_dist"], rtol=1e-6,
                                           atol=1e-9, err_msg=q)
                # the projection moves mass between atoms and loses none
                np.testing.assert_allclose(z[q + "target_dist"].sum(1), 1.0, rtol=0, atol=1e-5,
                                           err_msg=q)
                curr = dist(net, torch.as_tensor(store["obs"][idx]), kind, A, N)
                curr = curr[rows, store["act"][idx], :]
                out_w = -(target * torch.log(curr + 1e-8)).sum(1)
                loss = (out_w * w).mean()
            else:
                curr = dist(net, torch.as_tensor(store["obs"][idx]), kind, A, N)
                curr = curr[rows, store["act"][idx], :].unsqueeze(2)
                target = ret.unsqueeze(1)
                diff = F.smooth_l1_loss(target.expand(-1, N, -1), curr.expand(-1, -1, N),
                                        reduction="none")
                huber = (diff * (tau_hat - (target - curr).detach().le(0.).float()).abs()) \
                    .sum(-1).mean(1)
                loss = (huber * w).mean()
                out_w = diff.detach().abs().sum(-1).mean(1)
            loss.backward()
            optim.step()
            np.testing.assert_allclose(loss.item(), float(z[q + "loss"]), rtol=1e-6, err_msg=q)
            np.testing.assert_allclose(out_w.detach().numpy(), z[q + "out_weight"], rtol=1e-6,
                                       atol=1e-6, err_msg=q)
            keys = dh.param_keys(z, q + "param_")
            for (name, p), k in zip(sorted(net.state_dict().items()), keys):
                np.testing.assert_allclose(p.numpy(), z[k], rtol=1e-6, atol=1e-9,
                                           err_msg=f"{q}{name}")
        # the recorded gap is the trace's own, and no f32 summation order can flip an action
        assert len(gaps) == 6
        np.testing.assert_allclose(min(gaps), float(z[tag + "_top2_gap"]), rtol=1e-3)
        assert float(z[tag + "_top2_gap"]) >= 1e-4, tag
    assert clamped["low"] and clamped["high"]  # both ends of the C51 support clamp returns


def test_new_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in ("tsrl_dist_select", "tsrl_c51_loss_fwd_bwd", "tsrl_qr_loss_fwd_bwd"):
        assert name in _C.EXPORTED
        assert f" {name}(" in header


def test_policies_are_exported_with_reference_attributes():
    from tianshou_amd.policy import C51Policy, DQNPolicy, QRDQNPolicy
    net = torch.nn.Linear(1, 1)
    c51 = C51Policy(net, None, num_atoms=21, v_min=-4.0, v_max=4.0, target_update_freq=2)
    assert isinstance(c51, DQNPolicy) and c51._target and c51.delta_z == 0.4
    assert isinstance(c51.support, torch.nn.Parameter) and not c51.support.requires_grad
    assert torch.equal(c51.support.data, torch.linspace(-4.0, 4.0, 21))
    qr = QRDQNPolicy(net, None, num_quantiles=17)
    assert isinstance(qr, DQNPolicy) and tuple(qr.tau_hat.shape) == (1, 17, 1)
    assert isinstance(qr.tau_hat, torch.nn.Parameter) and not qr.tau_hat.requires_grad
    tau = torch.linspace(0, 1, 18)
    assert torch.equal(qr.tau_hat.data.view(-1), (tau[:-1] + tau[1:]) / 2)
    assert C51Policy(net, None)._num_atoms == 51 and QRDQNPolicy(net, None)._num_quantiles == 200
    with pytest.raises(AssertionError):
        C51Policy(net, None, num_atoms=1)
    with pytest.raises(AssertionError):
        C51Policy(net, None, v_min=1.0, v_max=1.0)
    with pytest.raises(AssertionError):
        QRDQNPolicy(net, None, num_quantiles=1)
    # CPU policies run the reference's torch formulation: [b, A, N] outputs reduce to Q-values
    logits = torch.rand(5, 3, 21)
    assert torch.equal(c51._greedy_act(logits), (logits * c51.support).sum(2).argmax(1))


def test_select_cases_exclude_at_most_one_percent_of_rows():
    """tests/test_gpu_dist_dqn.py compares tsrl_dist_select's action with the f64 argmax on
    the rows whose f64 top-two relative gap is >= 1e-6: with its seeds the f64 reference alone
    leaves out at most 1 % of the rows of any case."""
    from tests import test_gpu_dist_dqn as g
    for b in g.BS:
        for A in g.AS:
            for N in g.NS:
                for mode in ("c51", "qr"):
                    sel, _, w = g.select_inputs(b, A, N, mode)
                    gap = g.top2_rel_gap(g.q_f64(sel, w))
                    out = int((gap < 1e-6).sum())
                    assert out <= b // 100, (b, A, N, mode, out)
