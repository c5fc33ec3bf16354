"""CQLPolicy and TD3BCPolicy without a device: the C ABI's declarations, the torch formulation
(``fused = False``) replaying tests/golden/cont_offline.npz from the recorded indices and draws,
and the margins gen_cont_offline asserted on the reference alone."""
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests import cont_offline_common as cc
from tests.conftest import ROOT
from tianshou_amd import _C
from tianshou_amd.data.batch import Batch

SYMBOLS = ("tsrl_cql_expand", "tsrl_cql_target", "tsrl_cql_loss_fwd_bwd",
           "tsrl_td3bc_actor_loss_fwd_bwd")
TAGS = ("cql_lagrange", "cql_clamped", "cql_plain", "td3bc")


@pytest.fixture(scope="module")
def rec(golden_dir):
    return cc.recording(golden_dir)


def test_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for s in SYMBOLS:
        assert s in _C.EXPORTED and f"int {s}(" in header


@pytest.mark.parametrize("tag", TAGS)
def test_torch_formulation_replays_the_recording(rec, tag):
    """fused = False on the CPU (TD3BC from the recorded returns: the n-step kernel that makes
    them runs on the GPU only): the reference's loss keys and values (same library, possibly
    another summation split: rtol 1e-6) and every parameter at the Adam bound."""
    z, cfg = rec
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
    policy = cc.make_policy(z, cfg, tag, fused=False)
    policy.train()
    cc.feed_draws(policy, z, tag, cfg["updates"])
    for u in range(cfg["updates"]):
        idx = z[f"{tag}_u{u}_indices"]
        b = Batch(obs=store["obs"][idx], act=store["act"][idx], rew=store["rew"][idx],
                  done=store["terminated"][idx] | store["truncated"][idx],
                  obs_next=store["obs_next"][idx], info=Batch())
        if tag == "td3bc":
            b.returns = torch.as_tensor(z[f"{tag}_u{u}_returns"])
        cc.check_update(policy, z, tag, u, policy.learn(b), 1e-6)
    if tag == "cql_clamped":  # the clamp is active: the multiplier never moves
        assert policy.cql_log_alpha.item() == 0.0
    if tag == "td3bc":
        assert policy._cnt == cfg["updates"]


def test_recording_keeps_its_margins(rec):
    checks = rec[1]["checks"]
    for tag in TAGS:
        assert checks[tag]["reversed"] <= 2.5e-7
        assert tag == "td3bc" or checks[tag]["norm"] >= 1e-3
    assert checks["cql_lagrange"]["inside"] and not checks["cql_clamped"]["inside"]
    assert checks["cql_plain"]["clipped"] == 2 * rec[1]["updates"]
