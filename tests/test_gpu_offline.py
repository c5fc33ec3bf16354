"""csrc/offline.hip through the C ABI, and the three offline policies on the device path.

Kernels: outputs go into NaN-prefilled buffers and are compared with the f64 references of
tests/offline_common.py at the project's bounds: scalars rtol 1e-5,
gradients and priorities rtol 1e-4 with atol 1e-6 * max|ref|; tsrl_bcq_select exactly.

Policies: the recorded updates of tests/golden/offline.npz (the reference on CPU torch) on the
graph, eager and torch legs: sampled indices equal, returns rtol 1e-5 / atol 1e-6, losses
rtol 2e-5 / atol 1e-6, Adam parameters online and target rtol 1e-5 / atol 1e-6, the recorded
forward's actions equal; RMSprop at 4 x the torch formulation's measured deviation.
"""
import numpy as np
import pytest
import torch

from tests import offline_common as oc
from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy import offline as off

pytestmark = pytest.mark.gpu
LOG_TAU = float(np.log(0.3))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _d(x, dev):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _parts(b, k, dev):
    return _nan(dev, k * int(_C.lib().tsrl_dqn_num_partials(b)), dtype=torch.float64)


def _close(got, want, tag, rtol=1e-4):
    """Gradients and priorities: rtol 1e-4, atol 1e-6 * max|ref|; scalars: rtol 1e-5."""
    want = np.asarray(want)
    atol = 1e-6 * float(np.max(np.abs(want))) if rtol == 1e-4 else 0.0
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=rtol, atol=atol, err_msg=tag)


def _select(q, logits, log_tau, q_eval, paper, dev):
    b, A = q.shape
    act = torch.full((b,), -7, dtype=torch.int64, device=dev)
    val = _nan(dev, b)
    t = [_d(x, dev) for x in (q, logits, q_eval)]  # alive until the results are read
    _C.check(_C.lib().tsrl_bcq_select(
        _C.ptr(t[0]), _C.ptr(t[1]), log_tau, _C.ptr(t[2]), int(paper), b, A, _C.ptr(act),
        _C.ptr(val), _C.stream_ptr(dev)), "tsrl_bcq_select")
    return act.cpu().numpy(), val.cpu().numpy()


@pytest.mark.parametrize("paper", (False, True))
@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("A", oc.AS)
@pytest.mark.parametrize("b", oc.BS)
def test_bcq_select_is_exact(dev, b, A, kind, paper):
    q, q_eval = oc.table(kind, b, A, 1), oc.table("random", b, A, 2)
    logits = oc.table(kind, b, A, 3) * np.float32(1.0 if kind == "spread" else 1.5)
    act, val = _select(q, logits, LOG_TAU, q_eval, paper, dev)
    want_act, want_val = oc.select_ref(q, logits, LOG_TAU, q_eval, paper)
    np.testing.assert_array_equal(act, want_act)
    np.testing.assert_array_equal(val, want_val)
    if not paper:  # nothing is unlikely: the reference's line returns action 0 everywhere
        assert not _select(q, logits, -np.inf, q_eval, False, dev)[0].any()


@pytest.mark.parametrize("paper", (False, True))
def test_bcq_select_nan_and_a_tie_across_index_64(dev, paper):
    """A = 65.  Row 0: the maximal Q tied between actions 3 and 64, both allowed.  Row 1: a NaN
    logit makes the row maximum NaN, every ratio NaN, every action allowed.  Row 2: a NaN Q on an
    allowed action wins the paper argmax.  Row 3: a NaN Q on an unallowed action is not seen.
    Row 4: only action 64 is allowed."""
    q = np.tile(np.linspace(-1, 1, 65, dtype=np.float32), (5, 1))
    logits = np.zeros((5, 65), np.float32)
    logits[:, 0] = -9.0  # action 0 is unlikely except in row 1
    q[0, 3] = q[0, 64]
    logits[1, 7] = np.nan
    q[2, 40] = np.nan
    q[3, 0] = np.nan
    logits[4, :64] = -9.0
    act, val = _select(q, logits, LOG_TAU, q, paper, dev)
    want = [3, 64, 40, 64, 64] if paper else [1, 0, 1, 1, 64]
    assert act.tolist() == want
    np.testing.assert_array_equal(val, q[np.arange(5), want])
    np.testing.assert_array_equal(act, oc.select_ref(q, logits, LOG_TAU, q, paper)[0])


@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("A", oc.AS)
@pytest.mark.parametrize("b", oc.BS)
def test_bcq_loss_matches_f64(dev, b, A, kind):
    g = np.random.default_rng(b + A)
    q, logits = oc.table("random", b, A, 5) * np.float32(2), oc.table(kind, b, A, 6)
    act, ret = g.integers(0, A, b), g.normal(size=b).astype(np.float32)
    gq, gl, loss = _nan(dev, b, A), _nan(dev, b, A), _nan(dev, 4)
    t = [_d(x, dev) for x in (q, logits, act, ret)] + [_parts(b, 3, dev)]
    _C.check(_C.lib().tsrl_bcq_loss_fwd_bwd(
        _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(t[2]), _C.ptr(t[3]), 0.01, b, A, _C.ptr(gq),
        _C.ptr(gl), _C.ptr(t[4]), _C.ptr(loss), _C.stream_ptr(dev)), "tsrl_bcq_loss_fwd_bwd")
    want, want_gq, want_gl = oc.bcq_ref(q, logits, act, ret, 0.01)
    _close(loss, want, "losses", rtol=1e-5)
    _close(gq, want_gq, "grad_q")
    _close(gl, want_gl, "grad_logits")
    off_taken = np.ones((b, A), bool)
    off_taken[np.arange(b), act] = False
    assert not gq.cpu().numpy()[off_taken].any()


def _cql(curr, act, ret, tau, w, mqw, dev):
    b, A, N = curr.shape
    grad, prio, loss = _nan(dev, b, A, N), _nan(dev, b), _nan(dev, 3)
    t = [_d(x, dev) for x in (curr, act, ret, tau, w)] + [_nan(dev, 3 * b, dtype=torch.float64)]
    _C.check(_C.lib().tsrl_cql_qr_loss_fwd_bwd(
        _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(t[2]), _C.ptr(t[3]), _C.ptr(t[4]), mqw, b, A, N,
        _C.ptr(grad), _C.ptr(prio), _C.ptr(t[5]), _C.ptr(loss), _C.stream_ptr(dev)),
        "tsrl_cql_qr_loss_fwd_bwd")
    torch.cuda.synchronize()  # the inputs are released on return
    return grad, prio, loss


@pytest.mark.parametrize("N", oc.NS)
@pytest.mark.parametrize("A", oc.AS)
@pytest.mark.parametrize("b", oc.BS)
def test_cql_loss_matches_f64_and_the_qr_kernel(dev, b, A, N):
    kind, weighted = oc.KINDS[(b + A + N) % 3], (b + N) % 2 == 1  # spread over the cases
    g = np.random.default_rng(b * 7 + A * 3 + N)
    curr = oc.table(kind, b, A * N, 8).reshape(b, A, N)
    if kind == "spread":  # the quantile MEANS spread over 1e4; atoms of one action stay close
        curr = curr[:, :, :1] + g.normal(size=(b, A, N)).astype(np.float32)
    act = g.integers(0, A, b)
    ret = (curr[np.arange(b), act] + g.normal(size=(b, N)) * 1.5).astype(np.float32)
    tau = ((np.arange(N) + 0.5) / N).astype(np.float32)
    w = g.random(b).astype(np.float32) + 0.5 if weighted else None
    grad, prio, loss = _cql(curr, act, ret, tau, w, 2.5, dev)
    want, want_g, want_p = oc.cql_ref(curr, act, ret, tau, w, 2.5)
    _close(loss, want, "losses", rtol=1e-5)
    _close(grad, want_g, "grad")
    _close(prio, want_p, "prio")
    # min_q_weight = 0: tsrl_qr_loss_fwd_bwd bit for bit, zero off the taken rows
    grad0, prio0, loss0 = _cql(curr, act, ret, tau, w, 0.0, dev)
    g_qr, p_qr, l_qr = _nan(dev, b, A, N), _nan(dev, b), _nan(dev)
    t = [_d(x, dev) for x in (curr, act, ret, tau, w)] + [_nan(dev, b, dtype=torch.float64)]
    _C.check(_C.lib().tsrl_qr_loss_fwd_bwd(
        _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(t[2]), _C.ptr(t[3]), _C.ptr(t[4]), b, A, N,
        _C.ptr(g_qr), _C.ptr(p_qr), _C.ptr(t[5]), _C.ptr(l_qr), _C.stream_ptr(dev)),
        "tsrl_qr_loss_fwd_bwd")
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(grad0), bits(g_qr)) and torch.equal(bits(prio0), bits(p_qr))
    assert torch.equal(bits(loss0[1]), bits(l_qr))


@pytest.mark.parametrize("mode", list(off.CRR_MODES))
@pytest.mark.parametrize("kind", oc.KINDS)
@pytest.mark.parametrize("A", oc.AS)
@pytest.mark.parametrize("b", oc.BS)
def test_crr_loss_matches_f64(dev, b, A, kind, mode):
    c = oc.crr_case(kind, b, A)
    gq, gl, loss = _nan(dev, b, A), _nan(dev, b, A), _nan(dev, 4)
    k = oc.CRR
    t = [_d(c[n], dev) for n in ("q", "logits", "act", "t_logits", "t_q", "rew", "done")]
    parts = _nan(dev, 2 + 4 * int(_C.lib().tsrl_dqn_num_partials(b)), dtype=torch.float64)
    _C.check(_C.lib().tsrl_crr_loss_fwd_bwd(
        *(_C.ptr(x) for x in t), k["gamma"], off.CRR_MODES[mode], k["beta"], k["ub"], k["mqw"],
        b, A, _C.ptr(gq), _C.ptr(gl), _C.ptr(parts), _C.ptr(loss), _C.stream_ptr(dev)),
        "tsrl_crr_loss_fwd_bwd")
    want, want_gq, want_gl, _, _ = oc.crr_ref(mode=mode, **c, **k)
    _close(loss, want, "losses", rtol=1e-5)
    _close(gq, want_gq, "grad_q")
    _close(gl, want_gl, "grad_logits")


# -- policies against tests/golden/offline.npz -----------------------------------------------------
# RMSprop ("bcq_rms"), max |parameter - recorded| after each of the five updates, measured on an
# MI355X.  The torch formulation (fused = False), the bound's base:
TORCH_DEV = (5.96e-8, 5.96e-8, 5.96e-8, 6.71e-8, 6.71e-8)
# The fused legs in the same run, eager and graph alike: 2.98e-8 2.98e-8 4.47e-8 4.47e-8 5.96e-8.


@pytest.fixture(scope="module")
def rec(golden_dir):
    return oc.recording(golden_dir)


LEGS = {"graph": dict(graph_learn=True), "eager": dict(graph_learn=False),
        "torch": dict(fused=False)}


def _run_variant(z, cfg, dev, tag, check_state, **attrs):
    """The recorded update() calls of one variant from a device buffer filled with the recorded
    add() stream: sampled indices equal, returns rtol 1e-5 / atol 1e-6, losses rtol 2e-5 /
    atol 1e-6, the state by ``check_state(policy, prefix)``, then the recorded forward."""
    from tianshou_amd.data import VectorReplayBuffer
    policy, v = oc.make_policy(z, cfg, tag, dev, **attrs), cfg["variants"][tag]
    buf = VectorReplayBuffer(cfg["E"] * cfg["S"], cfg["E"], device=dev)
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        buf.add(Batch(**{key: z["add_" + key][sl] for key in (
            "obs", "act", "rew", "terminated", "truncated", "obs_next")}),
            buffer_ids=z["add_ids"][sl])
        o += int(k)
    process_fn, seen = policy.process_fn, []

    def rec_process(batch, buffer, indices):
        batch = process_fn(batch, buffer, indices)
        seen.append((np.array(indices, copy=True), batch.get("returns", None)))
        return batch

    policy.process_fn = rec_process
    np.random.seed(cfg["sample_seed"])
    for u in range(cfg["updates"]):
        res, q = policy.update(v["bs"], buf), f"{tag}_u{u}_"
        assert seen[u][0].tolist() == z[q + "indices"].tolist(), q
        if v["kind"] != "crr":
            np.testing.assert_allclose(torch.as_tensor(seen[u][1]).cpu().numpy().reshape(
                z[q + "returns"].shape), z[q + "returns"], rtol=1e-5, atol=1e-6, err_msg=q)
        np.testing.assert_allclose(list(res.values()), z[q + "losses"], rtol=2e-5, atol=1e-6,
                                   err_msg=q)
        check_state(policy, q + "sd_")
    policy.eval()
    act = policy(Batch(obs=torch.as_tensor(z["fixed_obs"], device=dev), info=Batch())).act
    assert act.cpu().tolist() == z[tag + "_fixed_act"].tolist()
    return policy


@pytest.mark.parametrize("leg", tuple(LEGS))
@pytest.mark.parametrize("tag", ("bcq", "bcq_shared", "cql", "crr_exp", "crr_binary"))
def test_update_matches_reference_adam(rec, dev, tag, leg, monkeypatch):
    z, cfg = rec
    calls, L = [], _C.lib()
    for s in ("tsrl_bcq_select", "tsrl_bcq_loss_fwd_bwd", "tsrl_cql_qr_loss_fwd_bwd",
              "tsrl_crr_loss_fwd_bwd"):
        monkeypatch.setattr(L, s, (lambda f, s=s: lambda *a: (calls.append(s), f(*a))[1])(
            getattr(L, s)))
    p = _run_variant(z, cfg, dev, tag, lambda policy, q: oc.assert_state(policy, z, q, q),
                     **LEGS[leg])
    if leg == "torch":
        assert not calls and p._flat is None
        return
    n, kind = cfg["updates"], cfg["variants"][tag]["kind"]
    assert p._flat is not None and p._flat.adam_bound(p.optim)
    assert bool(p._learn_graphs) == (leg == "graph") and not p._graph_failed
    # a replayed update makes no call: the warm-up update and the capture do
    assert sum(c.endswith("fwd_bwd") for c in calls) == (2 if leg == "graph" else n)
    if kind == "bcq":  # _target_q is one select launch per update, the last forward one more
        assert calls.count("tsrl_bcq_select") == n + 1


def test_update_matches_reference_rmsprop(rec, dev):
    """RMSprop's early steps amplify another f32 summation order; the bound is 4 x what the
    torch formulation of the same policy deviates from the same recording on the same GPU
    (TORCH_DEV, measured; this test prints both legs' figures again)."""
    z, cfg = rec
    devs = {}
    for leg in ("torch", "eager", "graph"):
        devs[leg] = []
        _run_variant(z, cfg, dev, "bcq_rms",
                     lambda policy, q, leg=leg: devs[leg].append(oc.state_dev(policy, z, q)),
                     **LEGS[leg])
        print(f"bcq_rms {leg}: max|dparam| per update", " ".join(f"{d:.3g}" for d in devs[leg]))
    for leg in ("eager", "graph"):
        for u, d in enumerate(devs[leg]):
            assert d <= 4 * TORCH_DEV[u], (leg, u, d)


def test_offline_trainer_runs_bcq_on_the_device_path(rec, dev):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import SyntheticVectorEnv
    from tianshou_amd.trainer import OfflineTrainer
    z, cfg = rec
    p, E, D, A = oc.make_policy(z, cfg, "bcq_shared", dev), 4, cfg["D"], cfg["A"]
    buf = VectorReplayBuffer(E * 64, E, device=dev)
    Collector(p, SyntheticVectorEnv(E, (D,), A, ep_len=16, device=dev, discrete=True),
              buf).collect(n_step=E * 48)
    test_c = Collector(p, SyntheticVectorEnv(2, (D,), A, ep_len=16, seed=5, device=dev,
                                             discrete=True))
    tr = OfflineTrainer(p, buffer=buf, test_collector=test_c, max_epoch=2, step_per_epoch=8,
                        episode_per_test=2, batch_size=32, verbose=False, show_progress=False)
    info = tr.run()
    assert tr.gradient_step == 16 and p._iter == 16 and "best_reward" in info
    assert p._learn_graphs and buf.fused_samples > 0
