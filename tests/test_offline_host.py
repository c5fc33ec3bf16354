"""The offline family without a device: the C ABI's declarations, the policies' reference
assertions, their torch formulation (``fused = False``) replaying tests/golden/offline.npz
from the recorded indices, the reference's BCQ action rule, OfflineTrainer's loop,
and the margins the CRR cases of tests/test_gpu_offline.py rely on."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests import offline_common as oc
from tests import trainer_script as ts
from tests.conftest import ROOT
from tianshou_amd import _C
from tianshou_amd.data.batch import Batch
from tianshou_amd.policy import DiscreteBCQPolicy, DiscreteCRRPolicy
from tianshou_amd.trainer import OfflineTrainer, offline_trainer

SYMBOLS = ("tsrl_bcq_select", "tsrl_bcq_loss_fwd_bwd", "tsrl_cql_qr_loss_fwd_bwd",
           "tsrl_crr_loss_fwd_bwd")
KEYS = {"bcq": ["loss", "loss/q", "loss/i", "loss/reg"], "cql": ["loss", "loss/qr", "loss/cql"],
        "crr": ["loss", "loss/actor", "loss/critic", "loss/cql"]}


@pytest.fixture(scope="module")
def rec(golden_dir):
    return oc.recording(golden_dir)


def _store(z, cfg):
    """The recorded add() stream laid out by buffer row (oracle/ref.py's ring arithmetic)."""
    vb = ref.VecBufferIndex(cfg["E"] * cfg["S"], cfg["E"])
    keys = ("obs", "act", "rew", "terminated", "truncated", "obs_next")
    store, o = {k: np.zeros((vb.maxsize,) + z["add_" + k].shape[1:], z["add_" + k].dtype)
                for k in keys}, 0
    for n in z["add_len"]:
        sl = slice(o, o + int(n))
        ptr, *_ = vb.add(z["add_rew"][sl], z["add_terminated"][sl], z["add_truncated"][sl],
                         z["add_ids"][sl])
        for k in keys:
            store[k][ptr] = z["add_" + k][sl]
        o += int(n)
    return store


def test_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert s in _C.EXPORTED and f"int {s}(" in header


def test_torch_formulation_replays_the_recording(rec):
    """fused = False on the CPU from the recorded indices (and the recorded returns: the n-step
    kernel that makes them runs on the GPU only): the reference's loss keys and values, and
    every parameter, online and target, after every update.  Same library, possibly another
    summation split: rtol 1e-6 on the losses, the Adam bound on the parameters."""
    z, cfg = rec
    store = _store(z, cfg)
    for tag, v in cfg["variants"].items():
        policy = oc.make_policy(z, cfg, tag, fused=False)
        assert json.loads(str(z[tag + "_loss_keys"])) == KEYS[v["kind"]]
        for u in range(cfg["updates"]):
            q = f"{tag}_u{u}_"
            idx = z[q + "indices"]
            assert len(idx) == v["bs"]
            b = Batch(obs=store["obs"][idx], act=store["act"][idx], info=Batch())
            if v["kind"] == "crr":
                b.obs_next, b.rew = store["obs_next"][idx], store["rew"][idx]
                b.done = store["terminated"][idx] | store["truncated"][idx]
            else:
                b.returns = torch.as_tensor(z[q + "returns"])
            got = policy.learn(b)
            assert list(got) == KEYS[v["kind"]]
            np.testing.assert_allclose(list(got.values()), z[q + "losses"], rtol=1e-6,
                                       err_msg=q)
            if v["optim"] == "adam":
                oc.assert_state(policy, z, q + "sd_", q)
            else:
                assert oc.state_dev(policy, z, q + "sd_") < 1e-6
        assert policy._iter == cfg["updates"]


def test_recording_keeps_its_margins(rec):
    """What gen_offline asserted on the reference alone, read back from the file; the recorded
    runs mask actions (BCQ) and clamp coefficients (CRR exp)."""
    checks, variants = rec[1]["checks"], rec[1]["variants"]
    for tag, c in checks.items():
        for key, least in (("ratio", 1e-3), ("gap", 1e-3), ("coef", 1e-3), ("adv", 1e-4)):
            assert c[key] is None or c[key] >= least, (tag, key)
        assert variants[tag]["optim"] == "rms" or c["reversed"] <= 2.5e-7
        assert c["masked"] > 0 or variants[tag]["kind"] != "bcq"
    assert checks["crr_exp"]["clamped"] > 0


def test_reference_assertions_and_the_first_allowed_action(rec):
    """The constructors' assertions; and the reference's (q - inf * mask).argmax: q = [1, 5, 3,
    9] with only the last action masked gives action 0, reference_argmax = False the best
    allowed one."""
    p = oc.make_policy(*rec, "crr_binary")
    assert p.actor_old is p.actor and p.critic_old is p.critic  # target_update_freq = 0
    with pytest.raises(AssertionError):
        DiscreteCRRPolicy(p.actor, p.critic, p.optim, policy_improvement_mode="other",
                          action_scaling=False)
    p = oc.make_policy(*rec, "bcq")
    with pytest.raises(AssertionError, match="target network"):
        DiscreteBCQPolicy(p.model, p.imitator, p.optim, target_update_freq=0)
    q, logits = torch.tensor([[1.0, 5.0, 3.0, 9.0]]), torch.tensor([[0.0, 0.0, 0.0, -5.0]])
    for paper, want in ((False, 0), (True, 1)):
        p.reference_argmax = not paper
        assert p._select(q, logits).tolist() == [want]
        assert oc.select_ref(q.numpy(), logits.numpy(), p._log_tau, q.numpy(),
                             paper)[0].tolist() == [want]


def test_offline_trainer_makes_one_update_per_step():
    log = []
    policy = ts.ScriptedPolicy(log, 0)
    test_c = ts.ScriptedCollector("test", policy, log, 1)
    buf = ts.ScriptedBuffer()
    buf.rows, buf.name = 40, "fixed"
    kw = dict(policy=policy, buffer=buf, test_collector=test_c, max_epoch=3, step_per_epoch=5,
              episode_per_test=2, batch_size=8, verbose=False, show_progress=False)
    info = OfflineTrainer(**kw).run()
    updates = [e[2] for e in log if e[1] == "update"]
    assert updates == [dict(sample_size=8, buffer="fixed", buffer_len=40)] * 15
    assert {"best_reward", "best_result", "duration", "test_step", "test_episode", "test_time",
            "test_speed", "train_time/model"} <= set(info) and "train_step" not in info
    tr = OfflineTrainer(**kw)
    epochs = list(tr)
    assert [e[0] for e in epochs] == [1, 2, 3] and tr.gradient_step == 15
    assert epochs[-1][1]["env_step"] == 15 * 8 and epochs[-1][1]["n/ep"] == 40
    assert set(offline_trainer(**kw)) == set(info)


@pytest.mark.parametrize("mode", ("exp", "binary", "all"))
def test_crr_cases_keep_their_margins(mode):
    """Every CRR case of the GPU test, on the f64 reference alone: |adv / beta| < 80, no
    coefficient within 1e-3 relative of the bound, no binary advantage within 1e-4 of zero;
    and the exp cases reach both sides of the bound."""
    below = above = 0
    for kind in oc.KINDS:
        for b in oc.BS:
            for a in oc.AS:
                c = oc.crr_case(kind, b, a)
                *_, z, e = oc.crr_ref(mode=mode, **c, **oc.CRR)
                assert oc.crr_margins_ok(z, e, mode, oc.CRR["beta"], oc.CRR["ub"]), (kind, b, a)
                below += int((e < oc.CRR["ub"]).sum())
                above += int((e > oc.CRR["ub"]).sum())
                if a == 1:
                    assert np.all(z == 0)
    assert below > 0 and above > 0
