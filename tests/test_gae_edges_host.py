"""The references of tests/test_gpu_gae_edges.py anchored on the CPU: the element-by-element
restatement ``gae_seq_ref`` (tests/gae_edges_common.py) equals the C oracle
(oracle.ref.compute_episodic_return) bit for bit on every finite case the GPU file runs, in
both value modes, and the reference goldens at their tests' tolerances; its non-finite
behaviour is the reference's; ``block_stats`` and ``rms_update_ref`` agree with NumPy."""
import os

import numpy as np
import pytest

from oracle import ref

from . import gae_edges_common as gc


def _oracle(c, scale):
    """The C oracle on a case: the forced row ends and the extra flags go in as unfinished
    indices, the scaled f64 values as v_s / v_s_ (a2c.py:98-100)."""
    n = c["n"]
    unfinished = np.flatnonzero(gc.end_flags(np.zeros(n), np.zeros(n), c["extra"], n,
                                             c["row_len"]))
    vs, vn = c["vs"], c["vn"]
    if scale is not None:
        vs, vn = vs.astype(np.float64) * scale, vn.astype(np.float64) * scale
    return ref.compute_episodic_return(c["rew"], c["term"], c["trunc"], np.arange(n), unfinished,
                                       vn, vs, c["gamma"], c["lam"])


def _seq(c, scale):
    return gc.gae_seq_ref(c["vs"], c["vn"], c["rew"], c["term"], c["trunc"], c["extra"],
                          c["gamma"], c["lam"], c["row_len"], scale)


@pytest.mark.parametrize("scale", [None, gc.SCALE, 1e-4], ids=["f32", "scaled", "scaled-1e-4"])
def test_restatement_equals_c_oracle_bitwise(scale):
    """Every finite case of the GPU file (sections a-f), f32-value and f64-value mode; the
    f64-value cases of section h with scale 1.  A per-row scan with forced row ends and the
    oracle's whole-array scan with those ends flagged are the same numbers while everything is
    finite (c = 0 cuts the chain)."""
    cases = gc.finite_cases() + (gc.cases_h() if scale == gc.SCALE else [])
    assert len(cases) > 150
    for c in cases:
        s = scale
        if c["vs"].dtype == np.float64:
            s = 1.0
        adv, ret, adv32, ret32 = _seq(c, s)
        ret_o, adv_o = _oracle(c, s)
        assert np.isfinite(adv_o).all(), c["name"]
        assert adv.tobytes() == adv_o.tobytes(), c["name"]
        assert ret.tobytes() == ret_o.tobytes(), c["name"]
        assert adv32.tobytes() == adv_o.astype(np.float32).tobytes(), c["name"]
        want32 = ret_o if s is None else ret_o / s
        assert ret32.tobytes() == want32.astype(np.float32).tobytes(), c["name"]


def test_restatement_on_reference_goldens(golden_dir):
    """tests/golden/gae_random.npz (test_gae_random_golden_general_path: rtol = atol = 1e-11)
    and returns_known.npz (test_known_answers_device: 1e-12)."""
    z = np.load(os.path.join(golden_dir, "gae_random.npz"))
    for tag in ("full", "wrap", "part"):
        p = tag + "_"
        extra = np.isin(z[p + "indices"], z[p + "unfinished"]).astype(np.uint8)
        for scaled in (False, True):
            adv, ret, _, _ = gc.gae_seq_ref(
                z[p + "v_s"], z[p + "v_s_"], z[p + "rew"], z[p + "term"], z[p + "trunc"], extra,
                0.99, 0.95, 0, float(z[p + "scale"]) if scaled else None)
            np.testing.assert_allclose(adv, z[p + ("adv_scaled" if scaled else "adv")],
                                       rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(ret, z[p + ("returns_scaled" if scaled else "returns")],
                                       rtol=1e-11, atol=1e-11)
    z = np.load(os.path.join(golden_dir, "returns_known.npz"))
    for c in range(int(z["ncases"])):
        p = f"c{c}_"
        n = len(z[p + "rew"])
        extra = np.isin(z[p + "indices"], z[p + "unfinished"]).astype(np.uint8)
        assert z[p + "indices"].tolist() == list(range(n))
        # compute_episodic_return (base.py:371-383): v_s_ None -> zeros, v_s = roll(v_s_, 1),
        # both f64 here
        vn = z[p + "v_next"].astype(np.float64) if bool(z[p + "has_v"]) else np.zeros(n)
        vs = np.roll(vn * (z[p + "term"] == 0), 1)
        adv, ret, _, _ = gc.gae_seq_ref(vs, vn, z[p + "rew"], z[p + "term"], z[p + "trunc"],
                                        extra, float(z[p + "gamma"]), float(z[p + "lam"]), 0, 1.0)
        np.testing.assert_allclose(ret, z[p + "returns"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(adv, z[p + "adv"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("scale", [None, gc.SCALE], ids=["f32", "scaled"])
def test_nonfinite_whole_array_scan(scale):
    """The reference's _gae_return (tianshou/policy/base.py:490-497) is one loop over the whole
    batch, ``gae = delta[i] + discount[i] * gae`` with ``discount = (1.0 - end_flag) * (gamma *
    gae_lambda)`` (:492, :495): an end flag multiplies the running value by 0.0, and 0 * NaN =
    0 * inf = NaN, so it does not stop a non-finite value.  With delta = rew + v_s_ * gamma -
    v_s (:491) a NaN in rew, v_s or v_s_ makes every advantage at or before it NaN, whatever
    end flags lie between; a +inf gives +-inf (or NaN, v_s_ at the value mask's 0) at its own
    index and back to the nearest end flag before it, NaN from that flag on.  Every index
    after it is finite."""
    cases = gc.cases_g()
    assert len(cases) == 18
    for c in cases:
        where, pos, value = c["poison"]
        end = gc.end_flags(c["term"], c["trunc"], c["extra"], c["n"], 0)
        assert end[:pos].any() and (pos == c["n"] - 1 or end[pos + 1:].any()), c["name"]
        for out in _seq(c, scale):
            assert np.isfinite(out[pos + 1:]).all(), c["name"]
            assert not np.isfinite(out[:pos + 1]).any(), c["name"]
            if np.isnan(value):
                assert np.isnan(out[:pos + 1]).all(), c["name"]
            else:
                last_end = int(np.flatnonzero(end[:pos]).max())
                assert np.isnan(out[:last_end + 1]).all(), c["name"]
                # ret = adv + v_s is inf - inf = NaN at a poisoned v_s itself
                tail = out[last_end + 1:pos + (0 if where == "vs" else 1)]
                assert np.isinf(tail).all(), c["name"]


@pytest.mark.parametrize("row_len,envs", gc.ROWS_G)
def test_nonfinite_per_row_scan(row_len, envs):
    """The row path scans every row on its own from a carry of exactly 0.0 (csrc/gae.hip,
    gae_rows_kernel), so a non-finite value stays inside its row: at or before it there,
    finite everywhere else."""
    for c in gc.cases_g(row_len, envs):
        _, pos, _ = c["poison"]
        row0 = pos - pos % row_len
        for scale in (None, gc.SCALE):
            for out in _seq(c, scale):
                bad = ~np.isfinite(out)
                assert bad[row0:pos + 1].all(), c["name"]
                bad[row0:pos + 1] = False
                assert not bad.any(), c["name"]


def test_block_stats_and_rms_update_ref():
    """block_stats against NumPy's mean / var, rms_update_ref against oracle.ref.RMS (the
    restated RunningMeanStd.update), at rtol 1e-12: the fsum versions are the more exact."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(5000) * 3 + 2
    bounds = [(0, 1), (1, 9), (9, 2057), (2057, 5000)]
    for (lo, hi), (n, m, m2) in zip(bounds, gc.block_stats(x, bounds)):
        assert n == hi - lo
        np.testing.assert_allclose(m, x[lo:hi].mean(), rtol=1e-12)
        np.testing.assert_allclose(m2, x[lo:hi].var() * n, rtol=1e-12, atol=1e-300)
    host, state = ref.RMS(), (0.0, 1.0, 0.0)
    for k in range(3):
        d = rng.standard_normal(100 + 37 * k) + k
        host.update(d)
        state = gc.rms_update_ref(state, d)
        np.testing.assert_allclose(state, (host.mean, host.var, host.count), rtol=1e-12)


def test_partial_blocks_are_well_posed():
    """The inputs behind every per-block partial the GPU file checks: no block of the restated
    returns has a variance or a mean near zero, so the relative bounds there are meaningful."""
    for c in gc.cases_a() + gc.cases_a_big() + gc.cases_b() + gc.cases_c() + [gc.case_d()]:
        ret = _seq(c, gc.SCALE)[1]
        assert gc.blocks_well_posed(ret, gc.partial_bounds(c["n"], c["row_len"])), c["name"]


def test_partial_bounds_follow_the_documented_ranges():
    """partial_bounds: tiles of 2048 on the general path; on the row path whole rows packed
    into a tile while they fit, a longer row on its own -- the last range may be short."""
    assert gc.partial_bounds(2049, 0) == [(0, 2048), (2048, 2049)]
    assert gc.range_len_for(3) == 2046 and gc.range_len_for(24) == 2040
    assert gc.range_len_for(2048) == 2048 and gc.range_len_for(3000) == 3000
    assert gc.partial_bounds(2400, 24) == [(0, 2040), (2040, 2400)]
    assert gc.partial_bounds(2560, 32) == [(0, 2048), (2048, 2560)]


def test_rms_blocks_zero_entries():
    parts, data = gc.rms_blocks(257, 1, zero_interleaved=True)
    assert (parts[1::2, 0] == 0).all() and (parts[0::2, 0] > 0).all()
    assert parts[:, 0].sum() == len(data)
    sizes = parts[0::2, 0]
    assert len(set(sizes.tolist())) > 10  # unequal blocks
