"""oracle/actor_ref.py kept honest on the CPU: the f64 references that tests/test_gpu_actor_ref.py
holds csrc/policy.hip and csrc/collect.hip against, and the headroom a correct f32 evaluation
has under the tolerances asserted there.

Measured (x86-64, numpy f64 / torch f32 CPU):
  * counter_normal over 2^16 rows x 32 actions, seed 0x123456789ABC, step 0: mean -5.4e-4,
    std 0.99959 (the sampling error of 2^21 draws is 5e-4);
  * the f32 restatement: at most 2.27 ulp32 of max(|z|, 1), 5.3e-7 absolute;
  * torch-f32 actor against gauss_act_ref: at most 0.05 of (1e-5 + 1e-5 |want|), the worst at
    D = 1000.
"""
import numpy as np
import pytest
import torch

from oracle import actor_ref
from tests.actor_common import BOUND_CASE, SHAPE_CASES, layer_arrays, make_actor

SEED = 0x1234_5678_9ABC


def test_counter_normal_moments():
    z = actor_ref.counter_normal(SEED, 0, np.arange(1 << 16), 32)
    assert z.shape == (1 << 16, 32) and z.dtype == np.float64
    assert np.isfinite(z).all()
    print("counter_normal mean %.3e std %.6f" % (z.mean(), z.std()))
    assert abs(z.mean()) < 0.005
    assert abs(z.std() - 1.0) < 0.005
    # per action column too (a wrong branch or pair index would bias single columns)
    assert np.abs(z.mean(axis=0)).max() < 0.02
    assert np.abs(z.std(axis=0) - 1.0).max() < 0.02


def test_counter_normal_cells_are_distinct():
    """No two of (row < 4096, action < 32, step in {0, 1, 2}) share a draw: the 48 hash bits
    behind every (row, pair, step) are distinct, and a pair's two actions (cos and sin branch)
    differ unless the angle is exactly pi/4 or 5 pi/4 (u2 = 1/8, 5/8) or the radius is 0
    (u1 = 1, probability 2^-24 per draw: step 2, row 1600, pair 1 of this seed is one)."""
    rows = np.arange(4096)
    us = [actor_ref._hash_uniforms(SEED, s, rows, 32) for s in range(3)]
    bits = np.stack([(u1 * 2.0 ** 24).astype(np.int64) << 24 | (u2 * 2.0 ** 24).astype(np.int64)
                     for u1, u2 in us])
    assert np.unique(bits).size == bits.size == 3 * 4096 * 16
    z = np.stack([actor_ref.counter_normal(SEED, s, rows, 32) for s in range(3)])
    u1, u2 = (np.stack([u[i] for u in us]) for i in (0, 1))
    same = z[..., 0::2] == z[..., 1::2]
    assert (np.isin(u2[same], (0.125, 0.625)) | (u1[same] == 1.0)).all() and same.sum() <= 1
    # whole rows (what a row- or step-sharing mistake in a kernel would repeat) never coincide
    flat = z.reshape(-1, 32)
    assert np.unique(flat, axis=0).shape[0] == flat.shape[0]


def test_counter_normal_indexing():
    """The value of a cell depends on (seed, step, row, action) alone: not on which rows are
    asked for together, nor on A beyond the action's own pair."""
    full = actor_ref.counter_normal(SEED, 5, np.arange(100), 32)
    rows = np.array([99, 0, 37])
    assert np.array_equal(actor_ref.counter_normal(SEED, 5, rows, 32), full[rows])
    for A in (1, 2, 5, 31):
        assert np.array_equal(actor_ref.counter_normal(SEED, 5, np.arange(100), A), full[:, :A])
    assert not np.array_equal(actor_ref.counter_normal(SEED + 1, 5, rows, 4), full[rows, :4])
    # Box-Muller: each pair's radius is sqrt(-2 ln u1) of its own hash
    u1, u2 = actor_ref._hash_uniforms(SEED, 5, np.arange(100), 32)
    assert (u1 > 0).all() and (u1 <= 1).all() and (u2 >= 0).all() and (u2 < 1).all()
    r2 = full[:, 0::2] ** 2 + full[:, 1::2] ** 2
    np.testing.assert_allclose(r2, -2.0 * np.log(u1), rtol=1e-12, atol=1e-300)


def test_counter_normal_f32_restatement_within_2p5_ulp():
    """The bound test_gpu_actor_ref.py's 9 ulp device margin is taken over."""
    worst = 0.0
    for step in (0, 7):
        rows = np.arange(1 << 16)
        z = actor_ref.counter_normal(SEED, step, rows, 32)
        zf = actor_ref.counter_normal_f32(SEED, step, rows, 32)
        assert zf.dtype == np.float32
        err =np.abs(zf.astype(np.float64) - z) / np.spacing(
            np.maximum(np.abs(z), 1.0).astype(np.float32)).astype(np.float64)
        print("step %d: %.3f ulp32 of max(|z|, 1), %.3e absolute"
              % (step, err.max(), np.abs(zf - z).max()))
        worst = max(worst, err.max())
    assert worst <= 2.5


def test_ulp_err32():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert actor_ref.ulp_err32(up, 1.0) == 1.0
    assert actor_ref.ulp_err32(one, 1.0) == 0.0
    assert actor_ref.ulp_err32(np.float32(0.5), 0.5 + 2.0 ** -26) == pytest.approx(0.25)
    assert actor_ref.ulp_err32(np.float32(np.inf), np.inf) == 0.0
    assert np.isnan(actor_ref.ulp_err32(np.float32(np.nan), 1.0))
    assert actor_ref.ulp_err32(np.float32(-1.0), 1.0) == 2.0 ** 24


def test_map_action_ref():
    x = np.array([-np.inf, -2.0, -1.0, 0.0, 0.5, 1.0, 3.0, np.inf])
    assert np.array_equal(actor_ref.map_action(x, None), x)
    assert np.array_equal(actor_ref.map_action(x, "clip"),
                          [-1.0, -1.0, -1.0, 0.0, 0.5, 1.0, 1.0, 1.0])
    y = actor_ref.map_action(x, "clip", np.full(8, -2.0), np.full(8, 3.0))
    assert np.array_equal(y, [-2.0, -2.0, -2.0, 0.5, 1.75, 3.0, 3.0, 3.0])
    assert np.array_equal(actor_ref.map_action(x, "tanh"), np.tanh(x))
    assert np.isnan(actor_ref.map_action(np.array([np.nan]), "clip"))[0]
    with pytest.raises(ValueError):
        actor_ref.map_action(x, "clip", np.zeros(8), None)


@pytest.mark.parametrize("D,A", [(d, a) for d, a, _ in SHAPE_CASES + [BOUND_CASE]])
def test_f32_actor_has_headroom_under_1e5(D, A):
    """A correct f32 evaluation (torch CPU, a different summation order from either kernel's)
    sits at most a quarter of rtol = atol = 1e-5 away from gauss_act_ref."""
    from tianshou_amd.policy.fused_act import match_actor
    n = 70
    actor, _ = make_actor(D, A, "cpu", D + A)
    layers = match_actor(actor)
    assert layers is not None
    g = torch.Generator().manual_seed(n)
    obs = torch.randn(n, D, generator=g)
    eps = torch.randn(n, A, generator=g)
    with torch.no_grad():
        mu = actor.forward_mu(obs)
        act = eps.mul(actor.sigma_param.view(1, -1).exp().expand_as(mu)).add(mu)
    arrs = layer_arrays(layers)
    want_mu, _ = actor_ref.gauss_act_ref(obs.numpy(), *arrs, None, None)
    want, remap = actor_ref.gauss_act_ref(obs.numpy(), *arrs, eps.numpy(), "clip")
    assert np.array_equal(remap, np.clip(want, -1.0, 1.0))
    share = max((np.abs(mu.numpy() - want_mu) / (1e-5 + 1e-5 * np.abs(want_mu))).max(),
                (np.abs(act.numpy() - want) / (1e-5 + 1e-5 * np.abs(want))).max())
    print("D %d A %d: %.4f of the tolerance" % (D, A, share))
    assert share <= 0.25
