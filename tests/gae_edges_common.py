"""References and case builders shared by tests/test_gae_edges_host.py (CPU) and
tests/test_gpu_gae_edges.py (GPU): the GAE and ret_rms kernels of csrc/gae.hip at tile, row,
alignment and non-finite edges.  NumPy and the standard library only; nothing here touches a
device.

``gae_seq_ref`` restates the arithmetic of ``make_elem`` and the header of csrc/gae.hip (the
reference's tianshou/policy/base.py:371-383 and :490-497 under NumPy-2 promotion) one
separately rounded f64 / f32 operation at a time; tests/test_gae_edges_host.py pins it to the C
oracle bit for bit.
"""
import math

import numpy as np

TPB, EPT = 256, 8
TILE = TPB * EPT  # transitions per tile of csrc/gae.hip
GAMMA, LAM = 0.99, 0.95
SCALE = 1.37  # the value_scale of the scaled modes (test_gae_staged_rows_kernel's)


# ---------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------
def end_flags(term, trunc, extra, n, row_len):
    """c_i = 0 where this is set: term | trunc | extra | forced row end."""
    end = (np.asarray(term) != 0) | (np.asarray(trunc) != 0)
    if extra is not None:
        end = end | (np.asarray(extra) != 0)
    if row_len > 0:
        end = end | ((np.arange(1, n + 1) % row_len) == 0)
    return end


def gae_seq_ref(vs, vn, rew, term, trunc, extra, gamma, lam, row_len=0, scale=None):
    """(adv64, ret64, adv32, ret32).  scale None: the f32-value mode (vs, vn float32);
    a float: the f64-value mode (vs, vn float32 or float64, multiplied by scale; ret32 is
    ret64 / scale).  row_len 0: one scan over the whole array; > 0: an independent scan per
    row of row_len elements (a shorter last row included)."""
    n = len(rew)
    rew = np.asarray(rew, np.float64)
    mask = (np.asarray(term) == 0)
    end = end_flags(term, trunc, extra, n, row_len)
    gl = float(gamma) * float(lam)
    with np.errstate(all="ignore"):
        if scale is None:
            vs32, vn32 = np.asarray(vs, np.float32), np.asarray(vn, np.float32)
            assert vs32.dtype == np.asarray(vs).dtype and vn32.dtype == np.asarray(vn).dtype
            t = (vn32 * mask.astype(np.float32)) * np.float32(gamma)
            assert t.dtype == np.float32
            vs64 = vs32.astype(np.float64)
            delta = (rew + t.astype(np.float64)) - vs64
            div = 1.0
        else:
            s = float(scale)
            vs64 = np.asarray(vs).astype(np.float64) * s
            vn64 = (np.asarray(vn).astype(np.float64) * s) * mask.astype(np.float64)
            delta = (rew + vn64 * float(gamma)) - vs64
            div = s
    adv = np.empty(n, np.float64)
    d, e = delta.tolist(), end.tolist()
    out = [0.0] * n
    rows = [(0, n)] if row_len <= 0 else [(a, min(a + row_len, n)) for a in range(0, n, row_len)]
    for a, b in rows:
        g = 0.0  # Python floats: IEEE binary64, one rounding per operation, no FMA
        for i in range(b - 1, a - 1, -1):
            g = d[i] + (0.0 if e[i] else gl) * g
            out[i] = g
    adv[:] = out
    with np.errstate(all="ignore"):
        ret = adv + vs64
        ret32 = (ret / div).astype(np.float32) if scale is not None else ret.astype(np.float32)
        adv32 = adv.astype(np.float32)
    return adv, ret, adv32, ret32


def block_stats(ret64, block_bounds):
    """[(n, mean, M2)] per block [lo, hi): two passes, both sums exact (math.fsum)."""
    out = []
    for lo, hi in block_bounds:
        x = [float(v) for v in ret64[lo:hi]]
        if not x:
            out.append((0.0, 0.0, 0.0))
            continue
        m = math.fsum(x) / len(x)
        out.append((float(len(x)), m, math.fsum((v - m) * (v - m) for v in x)))
    return out


def blocks_well_posed(ret64, block_bounds):
    """The relative bounds on a block's mean and M2 mean something only where neither is near
    zero: every block of 5 or more returns has variance > 1e-3 and |mean| > 1e-3."""
    for n, m, m2 in block_stats(ret64, block_bounds):
        if n >= 5 and not (m2 / n > 1e-3 and abs(m) > 1e-3):
            return False
    return True


def rel_err(got, want, rtol=1e-10):
    """|got - want| in units of rtol * |want|; an exact zero must be met exactly."""
    if want == 0.0:
        assert got == 0.0
        return 0.0
    return abs(got - want) / (rtol * abs(want))


def rms_update_ref(state, data):
    """RunningMeanStd.update (tianshou/utils/statistics.py:93-114) of state = (mean, var,
    count) with the batch mean and var of ``data`` from math.fsum."""
    mean, var, count = (float(v) for v in state)
    x = [float(v) for v in data]
    bc = float(len(x))
    bm = math.fsum(x) / bc
    bv = math.fsum((v - bm) * (v - bm) for v in x) / bc
    delta = bm - mean
    tot = count + bc
    new_mean = mean + delta * bc / tot
    m_2 = var * count + bv * bc + delta ** 2 * count * bc / tot
    return new_mean, m_2 / tot, tot


def range_len_for(row_len):
    """The transitions one workgroup of the row path owns (tsrl_gae_num_partials: rows are
    packed into a tile while they fit, a longer row is its own range)."""
    return row_len if row_len >= TILE else (TILE // row_len) * row_len


def partial_bounds(n, row_len):
    r = TILE if row_len <= 0 else range_len_for(row_len)
    return [(a, min(a + r, n)) for a in range(0, n, r)]


# ---------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------
def base_inputs(n, seed, f64_values=False):
    """randn values, rand rewards (the inputs of tests/test_gpu_gae.py), no end flags."""
    rng = np.random.default_rng(seed)
    vt = np.float64 if f64_values else np.float32
    return dict(
        n=n, vs=rng.standard_normal(n).astype(vt), vn=rng.standard_normal(n).astype(vt),
        rew=rng.random(n), term=np.zeros(n, np.uint8), trunc=np.zeros(n, np.uint8),
        extra=None, gamma=GAMMA, lam=LAM, row_len=0)


def _case(name, n, seed, pos=None, kind="term", **kw):
    c = base_inputs(n, seed)
    c["name"] = name
    if pos is not None:
        pos = np.asarray(pos, np.int64)
        pos = pos[pos < n]
        if kind == "extra":
            c["extra"] = np.zeros(n, np.uint8)
        c[kind][pos] = 1
    c.update(kw)
    return c


SIZES_A = (1, 7, 8, 9, 2047, 2048, 2049, 3 * 2048, 3 * 2048 + 5)
N_CARRY2 = 257 * 2048 + 1  # 258 tiles: gae_carry_kernel per = 2, threads with empty ranges


def end_patterns(n):
    i = np.arange(n)
    return {
        "all": i,
        "i2047": [2047], "i2048": [2048], "i4095": [4095], "tile-edges": [2047, 2048, 4095],
        "mod8=7": i[i % 8 == 7], "mod8=0": i[i % 8 == 0], "wave-edge": i[i % 512 == 511],
    }


def cases_a():
    """General path: every size x every end pattern, the flags on term, trunc or extra."""
    out = []
    for n in SIZES_A:
        out.append(_case(f"a n={n} none", n, n))
        for pname, pos in end_patterns(n).items():
            if len(np.asarray(pos)[np.asarray(pos) < n]) == 0:
                continue
            for kind in ("term", "trunc", "extra"):
                out.append(_case(f"a n={n} {pname} {kind}", n, n + 17, pos, kind))
    return out


def cases_a_big():
    rng = np.random.default_rng(5)
    n = N_CARRY2
    pos = np.flatnonzero(rng.random(n) < 1e-4)  # segments of ~10000: carries cross tiles
    return [_case(f"a n={n} none", n, 3), _case(f"a n={n} sparse trunc", n, 4, pos, "trunc")]


ROWS_B = ((1, 5000), (3, 1500), (8, 600), (24, 100), (32, 80), (300, 20), (1000, 7),
          (2048, 3), (2052, 5), (3000, 4), (4096, 2))


def cases_b():
    """Row path: (row_len, envs) with ranges off the 8-element grid (3, 300, 2052), short last
    ranges (24 x 100, 32 x 80, 3 x 1500, ...), tiles inside a row (3000, 4096), random term /
    trunc, with and without extra."""
    out = []
    for row_len, envs in ROWS_B:
        n = row_len * envs
        for with_extra in (False, True):
            c = base_inputs(n, 100 + row_len)
            rng = np.random.default_rng(200 + row_len)
            u = rng.random(n)
            c["term"] = (u < 0.01).astype(np.uint8)
            c["trunc"] = ((u > 0.99)).astype(np.uint8)
            if with_extra:
                c["extra"] = ((u > 0.5) & (u < 0.51)).astype(np.uint8)
            c["row_len"] = row_len
            c["name"] = f"b row_len={row_len} envs={envs} extra={with_extra}"
            out.append(c)
    return out


def cases_c():
    """Ranges that are exactly one or two aligned 2048-tiles."""
    out = []
    for name, n, row_len in (("general 2 tiles", 2 * TILE, 0), ("rows 2048 x 3", 3 * TILE, TILE),
                             ("rows 4096 x 2", 4 * TILE, 2 * TILE)):
        c = base_inputs(n, 300 + n + row_len)
        u = np.random.default_rng(301 + n).random(n)
        c["term"] = (u < 0.005).astype(np.uint8)
        c["trunc"] = (u > 0.995).astype(np.uint8)
        c["row_len"] = row_len
        c["name"] = "c " + name
        out.append(c)
    return out


def case_d():
    n = 2 * TILE + 8
    c = base_inputs(n, 400)
    u = np.random.default_rng(401).random(n)
    c["term"] = (u < 0.01).astype(np.uint8)
    c["trunc"] = (u > 0.99).astype(np.uint8)
    c["extra"] = ((u > 0.5) & (u < 0.51)).astype(np.uint8)
    c["name"] = "d"
    return c


SCALES_E = (1.0, 1.37, 3.0, math.sqrt(0.0 + 1e-8), 1e4)


def cases_e():
    out = []
    for row_len, n in ((0, 3 * TILE + 5), (TILE, 2 * TILE), (300, 3000)):
        c = base_inputs(n, 500 + row_len)
        u = np.random.default_rng(501).random(n)
        c["term"] = (u < 0.01).astype(np.uint8)
        c["row_len"] = row_len
        c["name"] = f"e row_len={row_len}"
        out.append(c)
    return out


def cases_f_exact():
    """c = 0 everywhere: no carry is ever used."""
    n = 3 * TILE + 5
    return [_case("f lambda=0", n, 600, gamma=0.99, lam=0.0),
            _case("f gamma=0", n, 601, gamma=0.0, lam=0.95),
            _case("f all-end", n, 602, np.arange(n), "trunc")]


def cases_f_tol():
    n = 5 * TILE + 3
    big = _case("f rew=1e6 v=1e-3", n, 611, np.arange(n)[::997], "trunc")
    big["rew"] = big["rew"] * 1e6
    big["vs"] = (big["vs"] * np.float32(1e-3)).astype(np.float32)
    big["vn"] = (big["vn"] * np.float32(1e-3)).astype(np.float32)
    return [_case("f gamma=lambda=1", n, 610, gamma=1.0, lam=1.0), big]


N_G = 3 * TILE + 5
POS_G = {"mid-thread": TILE + 8 * 37 + 3, "tile-first": 2 * TILE, "last": N_G - 1}
ROWS_G = ((1000, 7), (TILE, 3))


def _poison(c, where, pos, value):
    c[where] = c[where].copy()
    c[where][pos] = value
    c["poison"] = (where, pos, value)


def cases_g(row_len=0, envs=0):
    """One NaN or +inf in rew, v_s or v_s_ at the middle of a thread's eight elements, the
    first element of a tile, or the last element; end flags at pos - 5 and pos + 5 (and random
    ones elsewhere), so flags lie both before and after it."""
    out = []
    n = N_G if row_len == 0 else row_len * envs
    if row_len == 0:
        positions = POS_G
    else:
        r = range_len_for(row_len)
        positions = {"mid-thread": r + 8 * 37 + 3, "tile-first": 2 * r if 2 * r < n else r,
                     "last": n - 1}
    for where in ("rew", "vs", "vn"):
        for vname, value in (("nan", np.nan), ("inf", np.inf)):
            for pname, pos in positions.items():
                c = base_inputs(n, 700 + row_len)
                u = np.random.default_rng(701).random(n)
                c["term"] = (u < 0.005).astype(np.uint8)
                c["trunc"] = (u > 0.995).astype(np.uint8)
                for q in (pos - 5, pos + 5):
                    if 0 <= q < n:
                        c["trunc"][q] = 1
                c["term"][pos] = 0
                c["trunc"][pos] = 0
                c["row_len"] = row_len
                _poison(c, where, pos, value)
                c["name"] = f"g row_len={row_len} {where} {vname} {pname}"
                out.append(c)
    return out


ROWLENS_H = (0, 5, 2048, 3000)
SIZES_H = (1, 2049, 6000)


def cases_h():
    out = []
    for row_len in ROWLENS_H:
        for n in SIZES_H:
            for with_extra in (False, True):
                c = base_inputs(n, 800 + n + row_len, f64_values=True)
                u = np.random.default_rng(801 + n).random(n)
                c["term"] = (u < 0.01).astype(np.uint8)
                c["trunc"] = (u > 0.99).astype(np.uint8)
                if with_extra:
                    c["extra"] = ((u > 0.5) & (u < 0.52)).astype(np.uint8)
                c["row_len"] = row_len
                c["name"] = f"h row_len={row_len} n={n} extra={with_extra}"
                out.append(c)
    return out


def finite_cases():
    """Every finite case of the GPU file, for the bit-for-bit anchor against the C oracle."""
    d = case_d()
    return (cases_a() + cases_a_big() + cases_b() + cases_c() + [d] + cases_e()
            + cases_f_exact() + cases_f_tol())


NPARTS_I = (1, 2, 255, 256, 257, 1000)


def rms_blocks(nparts, seed, zero_interleaved=False):
    """(partials [nparts, 3], data) of random blocks of unequal sizes; zero_interleaved: every
    odd entry has count 0 (and junk in its mean and M2, which a merge must ignore)."""
    rng = np.random.default_rng(seed)
    parts = np.zeros((nparts, 3), np.float64)
    data = []
    for i in range(nparts):
        if zero_interleaved and i % 2 == 1:
            parts[i] = (0.0, 123.0, 456.0)
            continue
        x = rng.standard_normal(int(rng.integers(1, 40))) * 2.0 + 3.0
        parts[i] = block_stats(x, [(0, len(x))])[0]
        data.append(x)
    return parts, np.concatenate(data)


# ---------------------------------------------------------------------------------------
# error measures (units of the bound)
# ---------------------------------------------------------------------------------------
def _finite_max(want):
    f = np.abs(want[np.isfinite(want)])
    return float(f.max()) if f.size else 0.0


def err_f64(got, want):
    """max |got - want| / (atol + rtol |want|), atol = rtol = 1e-10 * max(1, max |want|), over
    the finite entries of want; non-finite entries must match exactly (NaN where NaN, the same
    infinity)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    b = 1e-10 * max(1.0, _finite_max(want))
    return _err(got, want, b, b)


def err_f32(got, want):
    """The same for test_gpu_gae.py's _tol: rtol 1e-5, atol 1e-6 * max |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return _err(got, want, 1e-5, 1e-6 * max(_finite_max(want), 1e-30))


def _err(got, want, rtol, atol):
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[np.isinf(want)], want[np.isinf(want)])
    assert np.isfinite(got[fin]).all()
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / (atol + rtol * np.abs(want[fin]))))
