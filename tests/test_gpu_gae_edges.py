"""The GAE and ret_rms kernels (csrc/gae.hip) through the C ABI at tile, row, alignment and
non-finite edges, against the element-by-element f64 restatement of
tests/gae_edges_common.py (anchored to the C oracle by tests/test_gae_edges_host.py).

Every output (adv32, ret32, adv64, ret64, the Welford partials, the general path's workspace,
the ret_rms state) is a slice of a larger buffer with 16 guard elements on each side, prefilled
with a sentinel bit pattern no arithmetic produces; every launch asserts that the guards are
untouched and that every output element was written.

Tolerances (the project's own): f64 outputs atol = rtol = 1e-10 * max(1, max |ref|)
(test_gae_full_size_vs_c_oracle); f32 outputs rtol 1e-5, atol 1e-6 * max |ref|
(test_gpu_gae.py's _tol); folded statistics rtol 1e-10 (test_ret_rms_update); per-block
partials: n exact, mean rtol 1e-10, M2 rtol 1e-10 + atol 1e-10 * n * max |ret|^2, on inputs
whose restated block variance is asserted not to be near zero.  Assertions that are bit-exact
say so.  Every group prints its largest error in units of the bound; the docstrings quote the
figures of profiles/gae_edges_gpu_tests.log.
"""
import numpy as np
import pytest
import torch

from . import gae_edges_common as gc

pytestmark = pytest.mark.gpu

GUARD = 16
SENT = {torch.float32: (torch.int32, 0xFFC0DE01 - (1 << 32)),
        torch.float64: (torch.int64, 0xFFF8C0DE0000BEEF - (1 << 64))}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class Guarded:
    """n elements of dtype inside a sentinel-filled buffer, `off` elements past the 16-byte
    aligned position behind the left guard."""

    def __init__(self, dev, n, dtype, off=0):
        it, self.sent = SENT[dtype]
        self.ibuf = torch.full((n + 2 * GUARD + off,), self.sent, dtype=it, device=dev)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.ibuf.view(dtype)[self.lo:self.hi]
        assert self.ibuf.data_ptr() % 16 == 0

    def check(self, written=True, what=""):
        b = self.ibuf.cpu().numpy()
        assert (b[:self.lo] == self.sent).all() and (b[self.hi:] == self.sent).all(), \
            f"{what}: guard elements overwritten"
        inner = b[self.lo:self.hi] == self.sent
        if written:
            assert not inner.any(), f"{what}: {int(inner.sum())} outputs not written"
        else:
            assert inner.all(), f"{what}: a refused call wrote outputs"

    def numpy(self):
        return self.t.cpu().numpy()


def _up(dev, a, off=0):
    """The array on the device, `off` elements past an aligned allocation."""
    if a is None:
        return None
    src = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.zeros(len(a) + off, dtype=src.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[off:] = src.to(dev)
    return buf[off:]


def run_gae(dev, c, scale=None, parts=False, want32=True, want64=True, off=None):
    """One tsrl_gae call on case c.  off: {argument name: elements to misalign it by}."""
    from tianshou_amd import _C
    off = off or {}
    L, n, row_len = _C.lib(), c["n"], c["row_len"]
    inp = {k: _up(dev, c[k], off.get(k, 0)) for k in ("vs", "vn", "rew", "term", "trunc", "extra")}
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float64, device=dev)
    out = {}
    for name, dt, want in (("adv32", torch.float32, want32), ("ret32", torch.float32, want32),
                           ("adv64", torch.float64, want64), ("ret64", torch.float64, want64)):
        out[name] = Guarded(dev, n, dt, off.get(name, 0)) if want else None
    nparts = int(L.tsrl_gae_num_partials(n, row_len))
    assert nparts == len(gc.partial_bounds(n, row_len))
    if parts:
        out["parts"] = Guarded(dev, 3 * nparts, torch.float64)
    ws_bytes = int(L.tsrl_gae_workspace_bytes(n, row_len))
    assert ws_bytes == (0 if row_len else 24 * ((n + gc.TILE - 1) // gc.TILE))
    if ws_bytes:
        out["ws"] = Guarded(dev, ws_bytes // 8, torch.float64)
    p = lambda k: _C.ptr(out[k].t) if out.get(k) is not None else None  # noqa: E731
    rc = L.tsrl_gae(_C.ptr(inp["vs"]), _C.ptr(inp["vn"]), _C.ptr(inp["rew"]), _C.ptr(inp["term"]),
                    _C.ptr(inp["trunc"]), _C.ptr(inp["extra"]), n, row_len, _C.ptr(sc),
                    float(c["gamma"]), float(c["lam"]), p("adv32"), p("ret32"), p("adv64"),
                    p("ret64"), p("parts"), p("ws"), ws_bytes, _C.stream_ptr(dev))
    _C.check(rc, "tsrl_gae")
    torch.cuda.synchronize()
    res = {}
    for k, g in out.items():
        if g is not None:
            g.check(what=f"{c['name']} {k}")
            res[k] = g.numpy()
    if parts:
        res["parts"] = res["parts"].reshape(nparts, 3)
    return res


def seq(c, scale):
    return gc.gae_seq_ref(c["vs"], c["vn"], c["rew"], c["term"], c["trunc"], c["extra"],
                          c["gamma"], c["lam"], c["row_len"], scale)


def errs(res, ref):
    """(f64, f32) errors of a run against the restatement, in units of the bounds."""
    adv, ret, adv32, ret32 = ref
    e64 = e32 = 0.0
    if "adv64" in res:
        e64 = max(gc.err_f64(res["adv64"], adv), gc.err_f64(res["ret64"], ret))
    if "adv32" in res:
        # adv32 against the f64 advantage (as _tol does), ret32 against ret64 / scale = ret32's
        # own definition before the final rounding
        e32 = max(gc.err_f32(res["adv32"], adv), gc.err_f32(res["ret32"], ret32))
    return e64, e32


def parts_err(parts, ret, n, row_len):
    """Largest error of the per-block (n, mean, M2) against block_stats, in units of the
    bound; n exact.  The restated block variance is asserted away from zero."""
    bounds = gc.partial_bounds(n, row_len)
    assert gc.blocks_well_posed(ret, bounds), "degenerate block in the inputs"
    want = gc.block_stats(ret, bounds)
    rmax = float(np.abs(ret).max())
    worst = 0.0
    for got, (bn, bm, bm2) in zip(parts, want):
        assert got[0] == bn
        worst = max(worst, gc.rel_err(got[1], bm))
        worst = max(worst, abs(got[2] - bm2) / (1e-10 * bm2 + 1e-10 * bn * rmax * rmax))
    return worst


def fold_err(dev, parts, ret, state0=(0.0, 1.0, 0.0)):
    """tsrl_ret_rms_update over the kernel's partials against rms_update_ref of the restated
    returns (rtol 1e-10, count exact): the largest error in units of the bound."""
    got = run_rms(dev, parts, state0)
    want = gc.rms_update_ref(state0, ret)
    assert got[2] == want[2]
    return max(gc.rel_err(got[k], want[k]) for k in (0, 1))


def run_rms(dev, parts, state0):
    from tianshou_amd import _C
    st = Guarded(dev, 3, torch.float64)
    st.t.copy_(torch.tensor(state0, dtype=torch.float64))
    pt = _up(dev, np.ascontiguousarray(parts, np.float64).reshape(-1))
    _C.check(_C.lib().tsrl_ret_rms_update(_C.ptr(pt), len(parts), _C.ptr(st.t),
                                          _C.stream_ptr(dev)), "tsrl_ret_rms_update")
    torch.cuda.synchronize()
    st.check(what="ret_rms state")
    return st.numpy()


def _report(group, **figs):
    print(f"GAE-EDGES {group}: " + ", ".join(f"{k} {v:.3g}" for k, v in figs.items())
          + " (largest error / bound)")


MODES = {"f32": (None, False), "scaled": (gc.SCALE, False), "scaled+parts": (gc.SCALE, True)}


# ---------------------------------------------------------------------------------------
# a. general path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_general_path_sizes_and_ends(dev, mode):
    """n in {1, 7, 8, 9, 2047, 2048, 2049, 6144, 6149} x {no end, every element, i = 2047 /
    2048 / 4095, i % 8 == 7, i % 8 == 0, i % 512 == 511} x the flag on term / trunc / extra,
    through agg -> carry -> apply; with partials also the per-tile Welford triples and their
    ret_rms fold (the launch A2CPolicy._compute_returns makes for a wrapped buffer).
    Measured: f64 1.9e-6, f32 5.2e-3 (half an f32 ulp), partials 9.3e-6, fold 3.7e-6 of the
    bound."""
    scale, parts = MODES[mode]
    w64 = w32 = wp = wf = 0.0
    cases = gc.cases_a()
    for c in cases:
        res = run_gae(dev, c, scale, parts)
        ref = seq(c, scale)
        e64, e32 = errs(res, ref)
        w64, w32 = max(w64, e64), max(w32, e32)
        if parts:
            wp = max(wp, parts_err(res["parts"], ref[1], c["n"], 0))
            wf = max(wf, fold_err(dev, res["parts"], ref[1]))
    _report(f"a general {mode} ({len(cases)} cases)", f64=w64, f32=w32, partials=wp, fold=wf)
    assert max(w64, w32, wp, wf) <= 1.0


def test_general_path_258_tiles(dev):
    """n = 257 * 2048 + 1: 258 tiles, so gae_carry_kernel's threads own two tiles each and
    the threads past 129 none; one segment across every tile, and ~10000-element segments.
    Scaled with partials (the one mode).  Measured: f64 2.0e-6, f32 5.2e-3, partials 2.5e-6,
    fold 1.2e-6 of the bound."""
    w64 = w32 = wp = wf = 0.0
    for c in gc.cases_a_big():
        res = run_gae(dev, c, gc.SCALE, True)
        ref = seq(c, gc.SCALE)
        e64, e32 = errs(res, ref)
        w64, w32 = max(w64, e64), max(w32, e32)
        wp = max(wp, parts_err(res["parts"], ref[1], c["n"], 0))
        wf = max(wf, fold_err(dev, res["parts"], ref[1]))
    _report("a general 258 tiles", f64=w64, f32=w32, partials=wp, fold=wf)
    assert max(w64, w32, wp, wf) <= 1.0


def test_gae_device_is_the_same_call(dev):
    """policy.base.gae_device (unguarded outputs of its own) gives the bits of the direct
    call, general path with partials and row path."""
    from tianshou_amd import _C
    from tianshou_amd.policy.base import gae_device
    for c in (gc.cases_a()[-1], gc.cases_b()[-1]):
        res = run_gae(dev, c, gc.SCALE, True)
        t = {k: _up(dev, c[k]) for k in ("vs", "vn", "rew", "term", "trunc", "extra")}
        nparts = int(_C.lib().tsrl_gae_num_partials(c["n"], c["row_len"]))
        parts = torch.empty(3 * nparts, dtype=torch.float64, device=dev)
        sc = torch.tensor([gc.SCALE], dtype=torch.float64, device=dev)
        outs = gae_device(t["vs"], t["vn"], t["rew"], t["term"], t["trunc"], c["gamma"], c["lam"],
                          c["row_len"], t["extra"], sc, want_f64=True, ret_partials=parts)
        for k, o in zip(("adv32", "ret32", "adv64", "ret64"), outs):
            assert o.cpu().numpy().tobytes() == res[k].tobytes(), (c["name"], k)
        assert parts.cpu().numpy().tobytes() == res["parts"].tobytes()


# ---------------------------------------------------------------------------------------
# b. row path
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("want64", [True, False], ids=["unstaged", "staged-where-eligible"])
def test_row_path(dev, want64):
    """row_len in {1, 3, 8, 24, 32, 300, 1000, 2048, 2052, 3000, 4096} (ranges off the
    8-element grid, short last ranges at 24 x 100 and 32 x 80, tiles inside a row), with and
    without extra, scaled with partials, against the per-row restatement; the partials' blocks
    are tsrl_gae_num_partials' ranges.  want_f64 keeps the per-thread-load kernel; without it
    row_len 2048 and 4096 take the LDS-staged one.  Measured: f64 1.3e-6, f32 5.1e-3, partials
    2.1e-6, fold 3.0e-6 of the bound."""
    w64 = w32 = wp = wf = 0.0
    cases = gc.cases_b()
    for c in cases:
        res = run_gae(dev, c, gc.SCALE, True, want64=want64)
        ref = seq(c, gc.SCALE)
        e64, e32 = errs(res, ref)
        w64, w32 = max(w64, e64), max(w32, e32)
        wp = max(wp, parts_err(res["parts"], ref[1], c["n"], c["row_len"]))
        wf = max(wf, fold_err(dev, res["parts"], ref[1]))
    _report(f"b rows want_f64={want64} ({len(cases)} cases)", f64=w64, f32=w32, partials=wp,
            fold=wf)
    assert max(w64, w32, wp, wf) <= 1.0


def test_row_path_f32_values(dev):
    """The same row cases in the f32-value mode (gae_rows_kernel<false> and the staged
    kernel's).  Measured: f64 1.6e-6, f32 5.2e-3 of the bound."""
    w64 = w32 = 0.0
    for c in gc.cases_b():
        for want64 in (True, False):
            e64, e32 = errs(run_gae(dev, c, None, False, want64=want64), seq(c, None))
            w64, w32 = max(w64, e64), max(w32, e32)
    _report("b rows f32 values", f64=w64, f32=w32)
    assert max(w64, w32) <= 1.0


# ---------------------------------------------------------------------------------------
# c. partials of full tiles
# ---------------------------------------------------------------------------------------
def test_full_tile_partials(dev):
    """Ranges of exactly one or two aligned 2048-tiles: block_welford_full / chan_eq (the
    vector branch of gae_tile, and gae_tile_staged) against block_stats -- and the same inputs
    with v_s misaligned by one element, so that the scalar branch and block_welford_fast /
    chan run: partials, adv and ret are bit-identical across the three kernels' folds.
    (chan_eq equals chan at equal counts as its comment says; block_welford_fast folded the
    four waves in sequence where block_welford_full pairs them, which this test found; both
    pair them now.)  Measured: partials 1.2e-6 of the bound."""
    wp = 0.0
    for c in gc.cases_c():
        ref = seq(c, gc.SCALE)
        runs = {"vector": run_gae(dev, c, gc.SCALE, True),
                "scalar": run_gae(dev, c, gc.SCALE, True, off={"vs": 1})}
        if c["row_len"]:
            runs["staged"] = run_gae(dev, c, gc.SCALE, True, want64=False)
        for name, res in runs.items():
            wp = max(wp, parts_err(res["parts"], ref[1], c["n"], c["row_len"]))
            assert res["parts"].tobytes() == runs["vector"]["parts"].tobytes(), (c["name"], name)
            for k in ("adv32", "ret32"):
                assert res[k].tobytes() == runs["vector"][k].tobytes(), (c["name"], name, k)
    _report("c full-tile partials", partials=wp)
    assert wp <= 1.0


# ---------------------------------------------------------------------------------------
# d. alignment, one pointer at a time
# ---------------------------------------------------------------------------------------
OFFSETS_D = [(k, 1) for k in ("vs", "vn", "rew", "term", "trunc", "extra", "adv32", "ret32",
                              "adv64", "ret64")] + [(k, 4) for k in ("term", "trunc", "extra")]


@pytest.mark.parametrize("row_len", [0, gc.TILE + 4], ids=["general", "rows"])
def test_alignment_one_pointer_at_a_time(dev, row_len):
    """n = 2 * 2048 + 8; exactly one of the ten pointers one element off its 16-byte (u8: 8-byte)
    alignment (u8 inputs also 4 bytes off): each turns vec_ok off alone, and all four outputs
    (and the partials) are bit-identical to the aligned run's.  Also as rows of 2052."""
    c = dict(gc.case_d(), row_len=row_len)
    base = run_gae(dev, c, gc.SCALE, True)
    for k, o in OFFSETS_D:
        res = run_gae(dev, c, gc.SCALE, True, off={k: o})
        for name in ("adv32", "ret32", "adv64", "ret64", "parts"):
            assert res[name].tobytes() == base[name].tobytes(), (k, o, name)
    base = run_gae(dev, c, None)
    for k, o in OFFSETS_D:
        res = run_gae(dev, c, None, off={k: o})
        for name in ("adv32", "ret32", "adv64", "ret64"):
            assert res[name].tobytes() == base[name].tobytes(), (k, o, name)


# ---------------------------------------------------------------------------------------
# e. div_by
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", gc.SCALES_E)
def test_div_by_is_correctly_rounded(dev, scale):
    """ret32 == float32(ret64 / scale) bit for bit on the kernel's own ret64 (general path with
    full and partial tiles, unstaged rows), so the claim is tested apart from the scan's
    re-association; the staged kernel's ret32 has the same bits."""
    for c in gc.cases_e():
        res = run_gae(dev, c, scale)
        want = (res["ret64"] / scale).astype(np.float32)
        assert res["ret32"].tobytes() == want.tobytes(), c["name"]
        if c["row_len"] == gc.TILE:
            st = run_gae(dev, c, scale, want64=False)
            assert st["ret32"].tobytes() == want.tobytes(), c["name"]


# ---------------------------------------------------------------------------------------
# f. gamma / lambda extremes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "scaled"])
def test_no_carry_cases_are_bit_exact(dev, mode):
    """lambda = 0, gamma = 0, and every element an end: c = 0 everywhere, no carry is ever used,
    and all four outputs equal the restatement bit for bit (general path and rows of 300)."""
    scale = MODES[mode][0]
    for c0 in gc.cases_f_exact():
        for row_len in (0, 300):
            c = dict(c0, row_len=row_len)
            res = run_gae(dev, c, scale)
            for name, want in zip(("adv64", "ret64", "adv32", "ret32"), seq(c, scale)):
                assert res[name].tobytes() == want.tobytes(), (c["name"], row_len, name)


@pytest.mark.parametrize("mode", ["f32", "scaled"])
def test_long_undiscounted_segment_and_large_rewards(dev, mode):
    """gamma = lambda = 1 without an end over n = 5 * 2048 + 3 (the advantage is a plain sum
    over every tile), and rewards of 1e6 against values of 1e-3.  Measured: f64 1.2e-8, f32
    5.3e-3 of the bound."""
    scale = MODES[mode][0]
    w64 = w32 = 0.0
    for c in gc.cases_f_tol():
        e64, e32 = errs(run_gae(dev, c, scale), seq(c, scale))
        w64, w32 = max(w64, e64), max(w32, e32)
    _report(f"f extremes {mode}", f64=w64, f32=w32)
    assert max(w64, w32) <= 1.0


# ---------------------------------------------------------------------------------------
# g. non-finite inputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "scaled"])
def test_nonfinite_general_path(dev, mode):
    """One NaN / +inf in rew, v_s or v_s_ (middle of a thread's eight, first of a tile, last
    element; end flags before and after): isnan of every output equals the whole-array
    restatement's -- every element at or before it, across end flags and tiles -- the
    infinities are the same, and the finite entries stay within tolerance.
    Measured: f64 1.5e-6, f32 5.2e-3 of the bound."""
    scale = MODES[mode][0]
    w64 = w32 = 0.0
    for c in gc.cases_g():
        e64, e32 = errs(run_gae(dev, c, scale), seq(c, scale))  # errs asserts NaN / inf places
        w64, w32 = max(w64, e64), max(w32, e32)
    _report(f"g non-finite general {mode}", f64=w64, f32=w32)
    assert max(w64, w32) <= 1.0


@pytest.mark.parametrize("row_len,envs", gc.ROWS_G)
def test_nonfinite_row_path(dev, row_len, envs):
    """The same on the row path (two rows per workgroup at row_len 1000; row_len 2048 also
    through the staged kernel) against the per-row restatement: the non-finite value stays in
    its row.  Measured: f64 1.4e-6, f32 5.2e-3 of the bound."""
    w64 = w32 = 0.0
    for c in gc.cases_g(row_len, envs):
        for scale in (None, gc.SCALE):
            ref = seq(c, scale)
            for want64 in (True, False):
                e64, e32 = errs(run_gae(dev, c, scale, want64=want64), ref)
                w64, w32 = max(w64, e64), max(w32, e32)
    _report(f"g non-finite rows {row_len}", f64=w64, f32=w32)
    assert max(w64, w32) <= 1.0


# ---------------------------------------------------------------------------------------
# h. tsrl_gae_f64v
# ---------------------------------------------------------------------------------------
def run_f64v(dev, c):
    from tianshou_amd import _C
    L, n, row_len = _C.lib(), c["n"], c["row_len"]
    inp = {k: _up(dev, c[k]) for k in ("vs", "vn", "rew", "term", "trunc", "extra")}
    adv, ret = Guarded(dev, n, torch.float64), Guarded(dev, n, torch.float64)
    ws_bytes = int(L.tsrl_gae_workspace_bytes(n, row_len))
    ws = Guarded(dev, ws_bytes // 8, torch.float64) if ws_bytes else None
    _C.check(L.tsrl_gae_f64v(
        _C.ptr(inp["vs"]), _C.ptr(inp["vn"]), _C.ptr(inp["rew"]), _C.ptr(inp["term"]),
        _C.ptr(inp["trunc"]), _C.ptr(inp["extra"]), n, row_len, float(c["gamma"]),
        float(c["lam"]), _C.ptr(adv.t), _C.ptr(ret.t), _C.ptr(ws.t) if ws else None, ws_bytes,
        _C.stream_ptr(dev)), "tsrl_gae_f64v")
    torch.cuda.synchronize()
    for g in (adv, ret) + ((ws,) if ws else ()):
        g.check(what=c["name"])
    return adv.numpy(), ret.numpy()


def test_gae_f64v_direct(dev):
    """tsrl_gae_f64v on f64 values: row_len in {0, 5, 2048, 3000} (the row branch has no other
    caller) x n in {1, 2049, 6000} (rows cut short by n included) x with / without extra,
    against the f64-value restatement with scale 1.  Measured: f64 1.5e-6 of the bound."""
    w = 0.0
    for c in gc.cases_h():
        adv, ret = run_f64v(dev, c)
        radv, rret, _, _ = seq(c, 1.0)
        w = max(w, gc.err_f64(adv, radv), gc.err_f64(ret, rret))
    _report("h f64v", f64=w)
    assert w <= 1.0


# ---------------------------------------------------------------------------------------
# i. tsrl_ret_rms_update
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("zeros", [False, True], ids=["dense", "zero-count-interleaved"])
def test_ret_rms_update_direct(dev, zeros):
    """nparts in {1, 2, 255, 256, 257, 1000} (one partial per thread or fewer, then per = 2 and
    4 with threads whose range is empty), partials of random blocks of unequal sizes, also
    with every odd entry of count 0 (junk in its mean and M2), from the fresh DeviceScalarRMS
    state and after two earlier updates, against rms_update_ref: rtol 1e-10, count exact.
    Measured: 2.3e-6 of the bound."""
    from tianshou_amd.utils.statistics import DeviceScalarRMS
    fresh = tuple(DeviceScalarRMS(dev).state.cpu().tolist())
    assert fresh == (0.0, 1.0, 0.0)
    w = 0.0
    for nparts in gc.NPARTS_I:
        if zeros and nparts == 1:
            continue  # (all counts zero: test_ret_rms_update_all_zero_counts)
        parts, data = gc.rms_blocks(nparts, 900 + nparts, zeros)
        got, want = fresh, fresh
        for k in range(2):  # the two earlier updates, through the kernel and the reference
            p0, d0 = gc.rms_blocks(3 + 300 * k, 950 + k)
            got, want = tuple(run_rms(dev, p0, got)), gc.rms_update_ref(want, d0)
        for g0, w0 in ((fresh, fresh), (got, want)):
            g1, w1 = run_rms(dev, parts, g0), gc.rms_update_ref(w0, data)
            assert g1[2] == w1[2]
            w = max(w, max(gc.rel_err(g1[k], w1[k]) for k in (0, 1)))
    _report(f"i ret_rms zeros={zeros}", fold=w)
    assert w <= 1.0


@pytest.mark.parametrize("nparts", [1, 257])
def test_ret_rms_update_all_zero_counts(dev, nparts):
    """Partials whose counts are all 0 leave {mean, var, count} bit-identical (the b.n > 0
    guard), from the fresh state and from a used one."""
    parts = np.tile(np.array([0.0, 123.0, 456.0]), (nparts, 1))
    for state in ((0.0, 1.0, 0.0), (2.5, 0.75, 1234.0)):
        got = run_rms(dev, parts, state)
        assert got.tobytes() == np.array(state, np.float64).tobytes()


# ---------------------------------------------------------------------------------------
# j. refusals
# ---------------------------------------------------------------------------------------
def _last_error():
    from tianshou_amd import _C
    return _C.lib().tsrl_last_error().decode(errors="replace")


def test_tsrl_gae_refusals(dev):
    """n < 0, a null input, row_len < 0, ret_partials without value_scale, the general path
    with a null and with a too small workspace: each returns non-zero before any launch
    (every TSRL_CHECK_ARG of tsrl_gae precedes its first kernel), names tsrl_gae in
    tsrl_last_error and leaves the outputs' sentinel; n == 0 returns 0 with null pointers."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    c = gc.cases_a()[-1]
    n = c["n"]
    t = {k: _up(dev, c[k]) for k in ("vs", "vn", "rew", "term", "trunc")}
    sc = torch.tensor([gc.SCALE], dtype=torch.float64, device=dev)
    ws_bytes = int(L.tsrl_gae_workspace_bytes(n, 0))
    outs = [Guarded(dev, n, torch.float32), Guarded(dev, n, torch.float32),
            Guarded(dev, n, torch.float64), Guarded(dev, n, torch.float64),
            Guarded(dev, 3 * int(L.tsrl_gae_num_partials(n, 0)), torch.float64),
            Guarded(dev, ws_bytes // 8, torch.float64)]

    def call(n=n, row_len=0, scale=sc, parts=True, ws=True, ws_bytes=ws_bytes, **null):
        a = {k: (None if null.get(k) else _C.ptr(v)) for k, v in t.items()}
        return L.tsrl_gae(a["vs"], a["vn"], a["rew"], a["term"], a["trunc"], None, n, row_len,
                          _C.ptr(scale), 0.99, 0.95, *[_C.ptr(o.t) for o in outs[:4]],
                          _C.ptr(outs[4].t) if parts else None,
                          _C.ptr(outs[5].t) if ws else None, ws_bytes, s)

    bad = {"n < 0": dict(n=-1), "row_len < 0": dict(row_len=-1),
           "partials without scale": dict(scale=None),
           "null workspace": dict(ws=False), "small workspace": dict(ws_bytes=ws_bytes - 8)}
    bad.update({f"null {k}": {k: True} for k in t})
    for what, kw in bad.items():
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc != 0, what
        assert "tsrl_gae:" in _last_error(), (what, _last_error())
        for o in outs:
            o.check(written=False, what=what)
    assert L.tsrl_gae(None, None, None, None, None, None, 0, 0, None, 0.99, 0.95, None, None,
                      None, None, None, None, 0, s) == 0
    assert call() == 0  # the same arguments, unbroken, are accepted
    torch.cuda.synchronize()
    for o in outs:
        o.check(what="accepted call")


def test_tsrl_gae_f64v_refusals(dev):
    """The same for tsrl_gae_f64v (its row_len < 0 check is new with this test: a negative
    row_len used to run as the general path)."""
    from tianshou_amd import _C
    L, s = _C.lib(), _C.stream_ptr(dev)
    c = gc.cases_h()[-1]
    n = c["n"]
    t = {k: _up(dev, c[k]) for k in ("vs", "vn", "rew", "term", "trunc")}
    ws_bytes = int(L.tsrl_gae_workspace_bytes(n, 0))
    outs = [Guarded(dev, n, torch.float64), Guarded(dev, n, torch.float64),
            Guarded(dev, ws_bytes // 8, torch.float64)]

    def call(n=n, row_len=0, ws=True, ws_bytes=ws_bytes, **null):
        a = {k: (None if null.get(k) else _C.ptr(v)) for k, v in t.items()}
        return L.tsrl_gae_f64v(a["vs"], a["vn"], a["rew"], a["term"], a["trunc"], None, n,
                               row_len, 0.99, 0.95, _C.ptr(outs[0].t), _C.ptr(outs[1].t),
                               _C.ptr(outs[2].t) if ws else None, ws_bytes, s)

    bad = {"n < 0": dict(n=-1), "row_len < 0": dict(row_len=-1),
           "null workspace": dict(ws=False), "small workspace": dict(ws_bytes=ws_bytes - 8)}
    bad.update({f"null {k}": {k: True} for k in t})
    for what, kw in bad.items():
        rc = call(**kw)
        torch.cuda.synchronize()
        assert rc != 0, what
        assert "tsrl_gae_f64v" in _last_error(), (what, _last_error())
        for o in outs:
            o.check(written=False, what=what)
    assert L.tsrl_gae_f64v(None, None, None, None, None, None, 0, 0, 0.99, 0.95, None, None,
                           None, 0, s) == 0
    assert call() == 0
    torch.cuda.synchronize()
    for o in outs:
        o.check(what="accepted call")
