"""The obs-normalisation kernels (csrc/rms.hip, csrc/rms_exact.h) called directly, at their span,
block and count edges.

A. tsrl_rms_exact_update (DeviceRunningMeanStd(exact=True)) bit for bit against oracle.ref.RMS
   (itself pinned to the reference by tests/test_oracle.py): the chain() tails at n mod 32 / 64,
   every column-group shape and both load paths, a masked first update, spans past 4096 rows,
   the two-update call on its concurrent path (reset rows <= 512) and on its sequential fallback,
   f32 count conversion past 2^24, and launches enqueued back to back.
B. The default path -- tsrl_rms_merge, tsrl_rms_merge2, tsrl_rms_sum_partials2 -- against the
   Chan merge of statistics.py:93-114 restated in np.longdouble over the same f64 partials, the
   state rounded to f32 after each update; tsrl_rms_norm_rows bitwise against NumPy f32; and
   the env kernels' partials (the producers) against the rows they wrote.

Tolerance of B.  The kernels fold nblk f64 partials and merge in f64: relative to the exact
arithmetic on the same partials their batch variance is off by at most about
nblk * 2^-53 * (1 + mean^2 / var).  For benign columns (|mean| / std <= 3, and the opposed-means
case's 1e4) that is < 1e-10, far below half an f32 ulp (2^-24), so the f32 state may differ from
the rounded longdouble result by one f32 ulp at the most (a result that falls on a rounding
boundary); the count is exact.  Cancellation columns (constant; mean 1e4 with std 1e-2) lose
ss / bc - bm^2 to rounding in any f64 evaluation: their var may be off by
(nblk + 8) * 2^-52 * (ss / bc) per update, plus the ulp, and must stay finite and >= 0.
Every test prints the largest deviation it saw, in f32 ulps.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LD = np.longdouble
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _step_rows(rng, k, D):
    return (rng.standard_normal((k, D)) * 3 + 1).astype(F32)


def _reset_rows(rng, k, D):
    return (rng.standard_normal((k, D)) * 0.5 - 2).astype(F32)


# =========================================================================================
# A. exact path, bitwise against oracle.ref.RMS
# =========================================================================================
class _Exact:
    """A DeviceRunningMeanStd(exact=True) and the oracle side by side; every update is applied
    to both and compared bit for bit."""

    def __init__(self, D, dev):
        from oracle import ref
        from tianshou_amd.utils.statistics import DeviceRunningMeanStd
        self.D, self.dev = D, dev
        self.rms = DeviceRunningMeanStd(D, dev, exact=True)
        self.ref = ref.RMS()

    def load(self, mean, var, count):
        self.rms.load(mean, var, count)
        self.ref.mean, self.ref.var, self.ref.count = mean.copy(), var.copy(), int(count)

    def _arr(self, v):
        if isinstance(v, np.ndarray):
            assert v.dtype == F32, v.dtype  # the oracle stayed in the reference's f32
            return v
        return np.full(self.D, F32(v))  # the untouched initial python scalars

    def _ref_update(self, x, mask):
        rows = x if mask is None else x[mask]
        if len(rows):  # the reference never updates with zero rows
            self.ref.update(np.ascontiguousarray(rows))

    def check(self, snap=None, what=""):
        assert np.array_equal(self.rms.mean, self._arr(self.ref.mean)), f"mean {what}"
        assert np.array_equal(self.rms.var, self._arr(self.ref.var)), f"var {what}"
        assert self.rms.count == self.ref.count, f"count {what}"
        if snap is not None:
            assert np.array_equal(self.rms.snap_mean_t.cpu().numpy(), self._arr(snap[0])), \
                f"snap mean {what}"
            assert np.array_equal(self.rms.snap_var_t.cpu().numpy(), self._arr(snap[1])), \
                f"snap var {what}"

    def update(self, x, mask=None, x2=None, mask2=None, snapshot=False, xt=None, via_update=False,
               what=""):
        t = lambda a: None if a is None else torch.as_tensor(a, device=self.dev)  # noqa: E731
        xt = t(x) if xt is None else xt
        if via_update:
            assert x2 is None and not snapshot
            self.rms.update(xt, t(mask))
        else:
            self.rms.exact_update(xt, t(mask), t(x2), t(mask2), snapshot=snapshot)
        self._ref_update(x, mask)
        # copies: the state between the updates, whatever the oracle does to its arrays later
        snap = tuple(v.copy() if isinstance(v, np.ndarray) else v
                     for v in (self.ref.mean, self.ref.var))
        if x2 is not None:
            self._ref_update(x2, mask2)
        self.check(snap if snapshot else None, what)


def test_exact_chain_tails(dev):
    """One object, D = 8, row counts around the 32-row register blocks and the 64-row rounds of
    exact::chain, up to the full 4096-row span."""
    rng = np.random.default_rng(101)
    p = _Exact(8, dev)
    for i, k in enumerate((1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 159, 160, 4095,
                           4096)):
        p.update(_step_rows(rng, k, 8), via_update=bool(i & 1), what=f"k={k}")


@pytest.mark.parametrize("k", [300, 4096])
@pytest.mark.parametrize("D", [2, 3, 4, 7, 8, 9, 12, 20, 372])
def test_exact_column_groups(dev, k, D):
    """Full and partial 8-column groups: float4 loads (dim % 4 == 0 and a full group), the scalar
    loads of a partial last group and of dim % 4 != 0."""
    rng = np.random.default_rng(1000 * D + k)
    p = _Exact(D, dev)
    p.update(_step_rows(rng, k, D), snapshot=True, what="first")
    p.update(_reset_rows(rng, 37, D), what="second")


@pytest.mark.parametrize("k", [300, 4096])
def test_exact_misaligned_base(dev, k):
    """D = 8 rows starting 4 bytes into an allocation: dim % 4 == 0 but the base is not 16-byte
    aligned, so the scalar load path runs on a full column group."""
    rng = np.random.default_rng(77 + k)
    p = _Exact(8, dev)
    for j, rows in enumerate((_step_rows(rng, k, 8), _reset_rows(rng, k, 8))):
        flat = torch.empty(k * 8 + 1, dtype=torch.float32, device=dev)
        xt = flat[1:].view(k, 8)
        xt.copy_(torch.as_tensor(rows))
        assert xt.is_contiguous() and xt.data_ptr() % 16 == 4
        p.update(rows, xt=xt, what=f"update {j}")


@pytest.mark.parametrize("k", [300, 4096])
@pytest.mark.parametrize("prob", [0.0, 0.003, 0.5, 1.0])
def test_exact_masked_first_update(dev, k, prob):
    """A mask on the first update (the row list of build_list); no row selected leaves state and
    count as they were, bit for bit."""
    rng = np.random.default_rng(k + int(prob * 1000))
    D = 20
    p = _Exact(D, dev)
    mask = rng.random(k) < prob
    p.update(_step_rows(rng, k, D), mask=mask, snapshot=True, what="fresh state")
    if prob == 0.0:
        assert p.rms.count == 0 and np.array_equal(p.rms.mean, np.zeros(D, F32)) \
            and np.array_equal(p.rms.var, np.ones(D, F32))
    p.update(_reset_rows(rng, 37, D), what="unmasked")
    before = (p.rms.mean, p.rms.var, p.rms.count)
    mask = rng.random(k) < prob
    p.update(_step_rows(rng, k, D), mask=mask, snapshot=True, what="masked")
    p.update(_step_rows(rng, k, D), mask=mask, via_update=True, what="masked, update()")
    if prob == 0.0:
        assert np.array_equal(p.rms.mean, before[0]) and np.array_equal(p.rms.var, before[1]) \
            and p.rms.count == before[2]


@pytest.mark.parametrize("k", [4097, 8192, 9001])
@pytest.mark.parametrize("D", [8, 20])
@pytest.mark.parametrize("variant", ["all", "half", "second_span", "none"])
def test_exact_more_than_one_span(dev, k, D, variant):
    """k > 4096: the rows are streamed twice, span by span."""
    rng = np.random.default_rng(k * 3 + D + len(variant))
    p = _Exact(D, dev)
    p.update(_reset_rows(rng, 37, D), what="prior")
    mask = {"all": None, "half": rng.random(k) < 0.5, "none": np.zeros(k, bool)}.get(variant)
    if variant == "second_span":
        mask = np.zeros(k, bool)
        mask[4096:] = rng.random(k - 4096) < 0.5
    p.update(_step_rows(rng, k, D), mask=mask, snapshot=True, what=variant)


def _exactly(rng, k, nd):
    m = np.zeros(k, bool)
    m[rng.choice(k, nd, replace=False)] = True
    return m


@pytest.mark.parametrize("D", [8, 20])
@pytest.mark.parametrize("nd", [0, 1, 511, 512, 513, 4096])
def test_exact_two_updates_reset_rows(dev, D, nd):
    """x2 / mask2 / snapshot at k = 4096: up to 512 reset rows run concurrently on wave 1, more
    take the sequential fallback (4096: every env resets in the same step)."""
    rng = np.random.default_rng(5 * nd + D)
    k = 4096
    p = _Exact(D, dev)
    p.update(_reset_rows(rng, 37, D), what="prior")
    for rep in range(2):  # the second call starts from the count the first published
        p.update(_step_rows(rng, k, D), x2=_reset_rows(rng, k, D), mask2=_exactly(rng, k, nd),
                 snapshot=True, what=f"nd={nd} call {rep}")


@pytest.mark.parametrize("D", [8, 20])
@pytest.mark.parametrize("case", ["k2_512", "k2_513", "k2_4097", "masked_first", "two_spans_first"])
def test_exact_two_updates_other_shapes(dev, D, case):
    """mask2 = None on both sides of the side span, a second batch longer than build_list reaches
    (8 * 512 rows), a masked first update followed by a second one, and a first update of two
    spans followed by a second one."""
    rng = np.random.default_rng(D + len(case) * 31)
    k = 4096
    p = _Exact(D, dev)
    p.update(_reset_rows(rng, 37, D), what="prior")
    x = _step_rows(rng, k, D)
    if case == "masked_first":
        p.update(x, mask=rng.random(k) < 0.5, x2=_reset_rows(rng, k, D),
                 mask2=_exactly(rng, k, 100), snapshot=True, what=case)
    elif case == "two_spans_first":
        p.update(_step_rows(rng, 5000, D), x2=_reset_rows(rng, 5000, D),
                 mask2=_exactly(rng, 5000, 100), snapshot=True, what=case)
    elif case == "k2_4097":
        p.update(x, x2=_reset_rows(rng, 4097, D), mask2=rng.random(4097) < 0.1, snapshot=True,
                 what=case + " masked")
        p.update(x, x2=_reset_rows(rng, 4097, D), snapshot=True, what=case + " unmasked")
    else:
        p.update(x, x2=_reset_rows(rng, int(case[3:]), D), snapshot=True, what=case)


@pytest.mark.parametrize("count", [2 ** 24 + 1, 25165829, 30000001])
def test_exact_counts_past_2_24(dev, count):
    """Counts that f32 no longer holds exactly: the merge converts count and total to f32 like
    the reference's NEP-50 scalars (headline: from the second iteration on)."""
    rng = np.random.default_rng(count % 1000)
    D = 12
    p = _Exact(D, dev)
    p.load(rng.standard_normal(D).astype(F32), (rng.random(D) * 4 + 0.1).astype(F32), count)
    p.check(what="load")
    for k in (4096, 37, 1, 5000):
        p.update(_step_rows(rng, k, D), snapshot=True, what=f"count {count} k={k}")
    assert p.rms.count == count + 4096 + 37 + 1 + 5000


def test_exact_back_to_back_launches(dev):
    """20 launches over 47 workgroups with no host synchronisation in between: each reads the
    count its predecessor published and the ticket ends re-armed."""
    rng = np.random.default_rng(20)
    D, k, n = 376, 300, 20
    p = _Exact(D, dev)
    xs = [(_step_rows if i % 2 == 0 else _reset_rows)(rng, k, D) for i in range(n)]
    masks = [rng.random(k) < 0.5 if i % 3 == 2 else None for i in range(n)]
    xt = torch.as_tensor(np.stack(xs), device=dev)
    mt = [None if m is None else torch.as_tensor(m, device=dev) for m in masks]
    torch.cuda.synchronize()
    for i in range(n):
        p.rms.exact_update(xt[i], mt[i])
    for x, m in zip(xs, masks):
        p._ref_update(x, m)
    p.check(what="after 20 launches")
    assert int(p.rms.ticket_t.item()) == 0


def test_exact_refuses_one_column(dev):
    """dim == 1 cannot be the reference's arithmetic (NumPy sums one column pairwise): the C
    entry returns the argument error before any launch."""
    from tianshou_amd import _C
    x = torch.zeros(4, 1, device=dev)
    m, v = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    c = torch.zeros(1, dtype=torch.float64, device=dev)
    tk = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _C.lib().tsrl_rms_exact_update(_C.ptr(x), None, 4, None, None, 0, 1, _C.ptr(m),
                                        _C.ptr(v), _C.ptr(c), None, None, _C.ptr(tk),
                                        _C.stream_ptr(dev))
    assert rc == 1  # hipErrorInvalidValue
    with pytest.raises(_C.TsrlError, match="dim == 1"):
        _C.check(rc, "tsrl_rms_exact_update")
    torch.cuda.synchronize()
    assert float(c.item()) == 0.0 and int(tk.item()) == 0


# =========================================================================================
# B. default path against the longdouble restatement
# =========================================================================================
ROWS = 16  # rows per partial block (tsrl_env_num_partials)


def _partials(x):
    """[k, D] f32 rows -> [nblk, D, 2] f64 (sum, sum of squares) per block of 16 rows."""
    k, D = x.shape
    nblk = (k + ROWS - 1) // ROWS
    xd = np.zeros((nblk * ROWS, D), np.float64)
    xd[:k] = x
    xb = xd.reshape(nblk, ROWS, D)
    return np.ascontiguousarray(np.stack([xb.sum(1), (xb * xb).sum(1)], axis=-1))


def _fold(p):
    """Column sums of [nblk, D, 2] partials in longdouble -> (s, ss)."""
    t = p.astype(LD).sum(0)
    return t[:, 0], t[:, 1]


def _chan(state, s, ss, bc):
    """RunningMeanStd.update (statistics.py:93-114) from batch sums in longdouble; the state
    (f32 mean, f32 var, int count) rounded to f32 as the reference stores it.  Also returns
    the batch second moment ss / bc (the scale of the cancellation bound)."""
    mean, var, cnt = state
    if bc == 0:
        return state, np.zeros(len(mean), LD)
    m0, v0, c0, n = mean.astype(LD), var.astype(LD), LD(cnt), LD(bc)
    tot = c0 + n
    bm = s / n
    bv = np.maximum(ss / n - bm * bm, LD(0))  # a variance: >= 0 in exact arithmetic
    delta = bm - m0
    nm = m0 + delta * n / tot
    m2 = v0 * c0 + bv * n + delta * delta * c0 * n / tot
    return (nm.astype(F32), (m2 / tot).astype(F32), cnt + int(bc)), ss / n


def _ulps(got, want):
    sp = np.spacing(np.maximum(np.abs(want), np.finfo(F32).tiny)).astype(np.float64)
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / sp))


def _one_ulp(got, want, what, slack=None):
    """got within one f32 ulp of the rounded reference (widened by slack, an absolute f64 bound
    per column, for cancellation columns); returns the deviation in ulps."""
    assert got.dtype == F32 and want.dtype == F32
    lo = np.nextafter(want, F32(-np.inf)).astype(np.float64)
    hi = np.nextafter(want, F32(np.inf)).astype(np.float64)
    if slack is not None:
        lo, hi = lo - slack, hi + slack
    g = got.astype(np.float64)
    bad = ~((g >= lo) & (g <= hi))
    assert not bad.any(), (what, np.flatnonzero(bad)[:8], got[bad][:8], want[bad][:8])
    return _ulps(got, want)


class _Dev:
    """Raw device state of one statistics object, driven through the C entry points."""

    def __init__(self, dim, dev, state=None):
        self.dim, self.dev = dim, dev
        mean, var, cnt = state if state is not None else (np.zeros(dim, F32), np.ones(dim, F32),
                                                          0)
        self.mean = torch.as_tensor(mean.copy(), device=dev)
        self.var = torch.as_tensor(var.copy(), device=dev)
        self.count = torch.full((1,), float(cnt), dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.snap_mean = torch.full((dim,), float("nan"), device=dev)
        self.snap_var = torch.full((dim,), float("nan"), device=dev)

    def up(self, a):
        return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def merge(self, p, nblk, mask, k, batch_count=None):
        from tianshou_amd import _C
        pt, mt = self.up(p), self.up(mask)
        bt = None if batch_count is None else torch.tensor([float(batch_count)],
                                                           dtype=torch.float64, device=self.dev)
        _C.check(_C.lib().tsrl_rms_merge(_C.ptr(pt), nblk, self.dim, _C.ptr(mt), k, _C.ptr(bt),
                                         _C.ptr(self.mean), _C.ptr(self.var),
                                         _C.ptr(self.count), _C.ptr(self.ticket),
                                         _C.stream_ptr(self.dev)), "tsrl_rms_merge")
        return self.read()

    def merge2(self, p1, p2, bd, nblk, k, k_dev=None):
        """p1 / p2 / bd / k_dev: host arrays (uploaded) or device tensors (used as they are)."""
        from tianshou_amd import _C
        t = [a if isinstance(a, torch.Tensor) else self.up(a) for a in (p1, p2, bd)]
        if k_dev is not None and not isinstance(k_dev, torch.Tensor):
            k_dev = torch.tensor([float(k_dev)], dtype=torch.float64, device=self.dev)
        _C.check(_C.lib().tsrl_rms_merge2(
            _C.ptr(t[0]), _C.ptr(t[1]), _C.ptr(t[2]), nblk, self.dim, k, _C.ptr(self.mean),
            _C.ptr(self.var), _C.ptr(self.count), _C.ptr(self.snap_mean), _C.ptr(self.snap_var),
            _C.ptr(self.ticket), _C.ptr(k_dev), _C.stream_ptr(self.dev)), "tsrl_rms_merge2")
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        assert int(self.ticket.item()) == 0
        return self.mean.cpu().numpy(), self.var.cpu().numpy(), float(self.count.item())

    def snap(self):
        return self.snap_mean.cpu().numpy(), self.snap_var.cpu().numpy()


def _state(rng, dim, count):
    return (rng.standard_normal(dim).astype(F32), (rng.random(dim) * 4 + 0.1).astype(F32), count)


def _cancel_rows(rng, k, dim):
    """Benign columns, with column 0 constant and, from dim 2 on, column 1 of mean 1e4 and std
    1e-2 (further such pairs every 16 columns)."""
    x = _step_rows(rng, k, dim)
    hard = np.zeros(dim, bool)
    for c in range(0, dim, 16):
        x[:, c] = F32(3.7)
        hard[c] = True
        if c + 1 < dim:
            x[:, c + 1] = (1e4 + 1e-2 * rng.standard_normal(k)).astype(F32)
            hard[c + 1] = True
    return x, hard


def _cancel_slack(nblk, m2nd):
    return (nblk + 8) * 2.0 ** -52 * m2nd.astype(np.float64)


@pytest.mark.parametrize("dim", [1, 6, 63, 64, 65, 376])
def test_merge_blocks_and_columns(dev, dim):
    """tsrl_rms_merge, mask = NULL: the 16-lane block loop (two blocks per lane and round, a
    tail block) and the 64-column workgroups; two merges in a row, the second on the count the
    first published."""
    rng = np.random.default_rng(dim)
    worst = 0.0
    for nblk in (1, 2, 15, 16, 17, 31, 32, 33, 47, 256):
        k = max(1, nblk * ROWS - 5)  # a partial last block
        st = _state(rng, dim, 1000) if nblk % 2 else None
        d = _Dev(dim, dev, st)
        want = st if st is not None else (np.zeros(dim, F32), np.ones(dim, F32), 0)
        for rows in (_step_rows(rng, k, dim), _reset_rows(rng, k, dim)):
            p = _partials(rows)
            assert p.shape[0] == nblk
            mean, var, cnt = d.merge(p, nblk, None, k)
            want, _ = _chan(want, *_fold(p), k)
            worst = max(worst, _one_ulp(mean, want[0], ("mean", nblk)),
                        _one_ulp(var, want[1], ("var", nblk)))
            assert cnt == want[2]
    print(f"tsrl_rms_merge dim {dim}: largest deviation from the longdouble merge "
          f"{worst:.2f} f32 ulp")


@pytest.mark.parametrize("dim", [1, 6, 63, 64, 65, 376])
def test_merge_mask_count_and_override(dev, dim):
    """The batch count of tsrl_rms_merge: the set bytes of a mask (any nonzero byte counts; the
    strided loop past 1024 rows), no byte set (nothing changes), and batch_count winning over a
    mask and k that say something else."""
    rng = np.random.default_rng(100 + dim)
    worst = 0.0
    st = _state(rng, dim, 777)
    masks = []
    for km in (5, 1024, 1025, 4096):
        mask = np.where(rng.random(km) < 0.5, rng.integers(1, 256, km), 0).astype(np.uint8)
        mask[km - 1] = 255  # the last byte of the strided loop counts
        masks.append(mask)
    for nblk in (15, 16, 17, 31, 32, 33):  # a masked count on both sides of the lane rounds
        n = nblk * ROWS - 5
        mask = np.zeros(2 * n, np.uint8)
        mask[rng.choice(2 * n, n, replace=False)] = rng.integers(1, 256, n)
        masks.append(mask)
    for mask in masks:
        km = len(mask)
        n = int((mask != 0).sum())
        p = _partials(_step_rows(rng, n, dim))
        d = _Dev(dim, dev, st)
        mean, var, cnt = d.merge(p, len(p), mask, km)
        want, _ = _chan(st, *_fold(p), n)
        worst = max(worst, _one_ulp(mean, want[0], ("mean", km)),
                    _one_ulp(var, want[1], ("var", km)))
        assert cnt == want[2] == 777 + n
        # the override: mask and k describe another batch
        d = _Dev(dim, dev, st)
        wrong = np.ones(km + 3, np.uint8)
        mean, var, cnt = d.merge(p, len(p), wrong, km + 3, batch_count=n)
        assert cnt == 777 + n
        worst = max(worst, _one_ulp(mean, want[0], ("mean, override", km)),
                    _one_ulp(var, want[1], ("var, override", km)))
        d = _Dev(dim, dev, st)
        mean, var, cnt = d.merge(p, len(p), None, n + 7, batch_count=n)
        assert cnt == 777 + n
        _one_ulp(mean, want[0], ("mean, override of k", km))
        _one_ulp(var, want[1], ("var, override of k", km))
        # no byte set: state and count bit for bit as before
        d = _Dev(dim, dev, st)
        mean, var, cnt = d.merge(p, len(p), np.zeros(km, np.uint8), km)
        assert np.array_equal(mean, st[0]) and np.array_equal(var, st[1]) and cnt == 777
    print(f"tsrl_rms_merge (masked) dim {dim}: largest deviation {worst:.2f} f32 ulp")


@pytest.mark.parametrize("dim", [6, 65, 376])
def test_merge_cancellation_columns(dev, dim):
    """Constant columns and columns of mean 1e4 / std 1e-2: ss / bc - bm^2 cancels; var stays
    finite, >= 0 (the bv < 0 clamp) and within the f64 rounding bound of the batch moment."""
    rng = np.random.default_rng(200 + dim)
    for nblk in (1, 17, 256):
        k = nblk * ROWS - 3
        x, hard = _cancel_rows(rng, k, dim)
        p = _partials(x)
        for st in (None, _state(rng, dim, 50)):
            d = _Dev(dim, dev, st)
            s0 = st if st is not None else (np.zeros(dim, F32), np.ones(dim, F32), 0)
            mean, var, cnt = d.merge(p, nblk, None, k)
            want, m2nd = _chan(s0, *_fold(p), k)
            assert np.isfinite(var).all() and (var >= 0).all() and np.isfinite(mean).all()
            _one_ulp(mean, want[0], ("mean", nblk))
            _one_ulp(var[~hard], want[1][~hard], ("var, benign", nblk))
            _one_ulp(var[hard], want[1][hard], ("var, cancelling", nblk),
                     _cancel_slack(nblk, m2nd[hard]))
            assert cnt == want[2]


def _merge2_case(rng, nblk, dim, pattern, cancel=False, opposed=False):
    """Partials of one vector step: k step rows in nblk blocks, blk_done per block, reset
    partials over the first blk_done rows of each done block, NaN where blk_done is 0 (slots
    the env kernel does not write).  Returns inputs and the two batches' sums."""
    k = max(1, nblk * ROWS - 3)
    hard = np.zeros(dim, bool)
    if cancel:
        x, hard = _cancel_rows(rng, k, dim)
        xr, _ = _cancel_rows(rng, nblk * ROWS, dim)
    else:
        x, xr = _step_rows(rng, k, dim), _reset_rows(rng, nblk * ROWS, dim)
        if opposed:  # batch means +100 / -100: the merged mean nearly cancels
            x = x - F32(1) + F32(100)
            xr = (xr + F32(2)) * F32(6) - F32(100)
    in_blk = np.minimum(ROWS, k - ROWS * np.arange(nblk))
    if pattern == "none":
        done = np.zeros(nblk, bool)
    elif pattern == "all":
        done = np.ones(nblk, bool)
    else:
        done = rng.random(nblk) < 0.05
        done[rng.integers(nblk)] = True
    bd = np.where(done, rng.integers(1, ROWS + 1, nblk), 0)
    bd = np.minimum(bd, in_blk)
    if pattern == "all" and not opposed:
        bd[0] = in_blk[0]
    if opposed:
        bd = in_blk.copy()  # as many reset rows as step rows
    p1 = _partials(x)
    p2 = np.full((nblk, dim, 2), np.nan)
    xrb = xr.reshape(nblk, ROWS, dim).astype(np.float64)
    for b in np.flatnonzero(bd):
        r = xrb[b, :bd[b]]
        p2[b, :, 0], p2[b, :, 1] = r.sum(0), (r * r).sum(0)
    s2 = np.where(bd[:, None, None] > 0, p2, 0.0)
    return dict(k=k, nd=int(bd.sum()), p1=p1, p2=p2, bd=bd.astype(np.float64), sums1=_fold(p1),
                sums2=_fold(s2), hard=hard)


def _check_merge2(d, got, c, st, slack_blocks=None):
    """got = (mean, var, count) after merge2 on case c from state st, d.snap() the state between
    the two updates; returns the largest deviation in ulps over the benign columns."""
    mean, var, cnt = got
    sm, sv = d.snap()
    for a in (mean, var, sm, sv):
        assert np.isfinite(a).all(), "a NaN slot of a block without reset rows reached the output"
    assert (var >= 0).all() and (sv >= 0).all()
    w1, m2a = _chan(st, *c["sums1"], c["k"])
    w2, m2b = _chan(w1, *c["sums2"], c["nd"])
    assert cnt == w2[2] == st[2] + c["k"] + c["nd"]
    hard, ok = c["hard"], ~c["hard"]
    worst = max(_one_ulp(sm, w1[0], "snap mean"), _one_ulp(mean, w2[0], "mean"))
    if ok.any():
        worst = max(worst, _one_ulp(sv[ok], w1[1][ok], "snap var"),
                    _one_ulp(var[ok], w2[1][ok], "var"))
    if hard.any():
        sl1 = _cancel_slack(slack_blocks, m2a[hard])
        _one_ulp(sv[hard], w1[1][hard], "snap var, cancelling", sl1)
        _one_ulp(var[hard], w2[1][hard], "var, cancelling",
                 sl1 + _cancel_slack(slack_blocks, m2b[hard]))
    if c["nd"] == 0:
        assert np.array_equal(mean, sm) and np.array_equal(var, sv)
    return worst


@pytest.mark.parametrize("dim", [1, 7, 8, 9, 376])
@pytest.mark.parametrize("pattern", ["none", "some", "all"])
def test_merge2_blocks_and_columns(dev, dim, pattern):
    """tsrl_rms_merge2: the 64-lane block loop and the 8-column workgroups; blocks without a
    reset row carry NaN in their reset slots and must be dropped."""
    rng = np.random.default_rng(300 + dim + len(pattern))
    worst = 0.0
    for nblk in (1, 63, 64, 65, 256):
        st = _state(rng, dim, 5000) if nblk % 2 else (np.zeros(dim, F32), np.ones(dim, F32), 0)
        c = _merge2_case(rng, nblk, dim, pattern)
        d = _Dev(dim, dev, st)
        got = d.merge2(c["p1"], c["p2"], c["bd"], nblk, c["k"])
        worst = max(worst, _check_merge2(d, got, c, st))
        # a second step on the same object reads the published count
        c2 = _merge2_case(rng, nblk, dim, pattern)
        st2 = (got[0], got[1], int(got[2]))
        got2 = d.merge2(c2["p1"], c2["p2"], c2["bd"], nblk, c2["k"])
        worst = max(worst, _check_merge2(d, got2, c2, st2))
    print(f"tsrl_rms_merge2 dim {dim} blk_done {pattern}: largest deviation {worst:.2f} f32 ulp")


@pytest.mark.parametrize("dim", [7, 376])
def test_merge2_k_dev_overrides_k(dev, dim):
    rng = np.random.default_rng(400 + dim)
    for nblk in (1, 65):
        st = _state(rng, dim, 321)
        c = _merge2_case(rng, nblk, dim, "some")
        d = _Dev(dim, dev, st)
        got = d.merge2(c["p1"], c["p2"], c["bd"], nblk, c["k"] + 11, k_dev=c["k"])
        _check_merge2(d, got, c, st)


@pytest.mark.parametrize("dim", [9, 376])
def test_merge2_cancellation_columns(dev, dim):
    rng = np.random.default_rng(500 + dim)
    for nblk in (1, 65, 256):
        for st in ((np.zeros(dim, F32), np.ones(dim, F32), 0), _state(rng, dim, 50)):
            c = _merge2_case(rng, nblk, dim, "all", cancel=True)
            d = _Dev(dim, dev, st)
            got = d.merge2(c["p1"], c["p2"], c["bd"], nblk, c["k"])
            _check_merge2(d, got, c, st, slack_blocks=nblk)


@pytest.mark.parametrize("dim", [8, 65])
def test_merge2_rounds_state_between_updates(dev, dim):
    """Step rows about +100, as many reset rows about -100, from an empty state: the merged mean
    nearly cancels, so its ulp is ~1e4 times finer than the snapshot's -- the second update
    must start from the snapshot ROUNDED to f32, as the reference's stored arrays are, or the
    mean is off by thousands of ulps.  (f64 error of the kernel: 2^-53 * 1e4 relative, still
    far below half an f32 ulp.)"""
    rng = np.random.default_rng(600 + dim)
    worst = 0.0
    for nblk in (4, 64):
        st = (np.zeros(dim, F32), np.ones(dim, F32), 0)
        c = _merge2_case(rng, nblk, dim, "all", opposed=True)
        d = _Dev(dim, dev, st)
        got = d.merge2(c["p1"], c["p2"], c["bd"], nblk, c["k"])
        assert np.abs(got[0]).max() < 5.0  # the case is what it claims
        worst = max(worst, _check_merge2(d, got, c, st))
    print(f"tsrl_rms_merge2 opposed means dim {dim}: largest deviation {worst:.2f} f32 ulp")


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 376])
@pytest.mark.parametrize("nblk", [1, 17, 256])
def test_sum_partials2_and_payload_route(dev, dim, nblk):
    """tsrl_rms_sum_partials2: the count thread sits at column index dim (the last lane of a
    wave at 63, the first of a new workgroup at 64); sums within nblk * 2^-53 relative of the
    longdouble sums; then merge2(nblk = 1,
    k_dev) on the payload -- DeviceRunningMeanStd.merge2's data-parallel route -- against the
    direct multi-block call."""
    from tianshou_amd import _C
    rng = np.random.default_rng(700 + dim * 3 + nblk)
    c = _merge2_case(rng, nblk, dim, "some")
    st = _state(rng, dim, 4321)
    direct = _Dev(dim, dev, st)
    got_d = direct.merge2(c["p1"], c["p2"], c["bd"], nblk, c["k"])
    u = _check_merge2(direct, got_d, c, st)

    route = _Dev(dim, dev, st)
    p1, p2, bd = route.up(c["p1"]), route.up(c["p2"]), route.up(c["bd"])
    out = torch.full((4 * dim + 2,), float("nan"), dtype=torch.float64, device=dev)
    _C.check(_C.lib().tsrl_rms_sum_partials2(_C.ptr(p1), _C.ptr(p2), _C.ptr(bd), nblk, dim,
                                             c["k"], _C.ptr(out), _C.stream_ptr(dev)),
             "tsrl_rms_sum_partials2")
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isfinite(o).all()
    assert o[4 * dim] == c["nd"] and o[4 * dim + 1] == c["k"]
    live = np.where(c["bd"][:, None, None] > 0, c["p2"], 0.0)
    for name, got, parts in (("step", o[:2 * dim], c["p1"]), ("reset", o[2 * dim:4 * dim], live)):
        want = parts.astype(LD).sum(0).reshape(-1)
        err = np.abs(got.astype(LD) - want)
        assert (err <= nblk * LD(2) ** -53 * np.abs(want)).all(), (name, float(err.max()))
    got_r = route.merge2(out[:2 * dim], out[2 * dim:4 * dim], out[4 * dim:], 1, 0,
                         k_dev=out[4 * dim + 1:])
    u = max(u, _check_merge2(route, got_r, c, st))
    assert got_r[2] == got_d[2]
    _one_ulp(got_r[0], got_d[0], "mean, payload route vs direct")
    _one_ulp(got_r[1], got_d[1], "var, payload route vs direct")
    for a, b, n in zip(route.snap(), direct.snap(), ("snap mean", "snap var")):
        _one_ulp(a, b, n + ", payload route vs direct")
    print(f"tsrl_rms_sum_partials2 + merge2 dim {dim} nblk {nblk}: largest deviation "
          f"{u:.2f} f32 ulp")


# -----------------------------------------------------------------------------------------
# tsrl_rms_norm_rows
# -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,dim", [(1, 1), (37, 6), (4096, 376), (6000, 376)])
def test_norm_rows_bitwise(dev, k, dim):
    """clip((x - mean) / sqrt(var + eps), +-clip) in f32, bit for bit NumPy's; (6000, 376) is
    more elements than the 8192 x 256 threads of the capped grid (the grid-stride loop)."""
    from tianshou_amd import _C
    rng = np.random.default_rng(800 + k + dim)
    x = _step_rows(rng, k, dim)
    far = rng.random((k, dim)) < 0.05
    x[far] *= F32(100)  # far enough out to clip
    x[0, 0] = F32(1e6)
    mean = rng.standard_normal(dim).astype(F32)
    var = (rng.random(dim) * 4 + 0.01).astype(F32)
    eps = F32(np.finfo(F32).eps)
    raw = (x - mean) / np.sqrt(var + eps)
    assert raw.dtype == F32 and np.abs(raw).max() > 10 and (k == 1 or np.abs(raw).min() < 10)
    xt, mt, vt = (torch.as_tensor(a, device=dev) for a in (x, mean, var))
    mask = rng.random(k) < 0.5
    mask[0] = True
    mk = torch.as_tensor(mask.astype(np.uint8) * 3, device=dev)  # any nonzero byte selects
    for clip, want in ((10.0, np.clip(raw, F32(-10), F32(10))), (0.0, raw)):
        out = torch.full((k, dim), -12345.0, device=dev)
        _C.check(_C.lib().tsrl_rms_norm_rows(_C.ptr(xt), None, k, dim, _C.ptr(mt), _C.ptr(vt),
                                             float(eps), clip, _C.ptr(out), _C.stream_ptr(dev)),
                 "tsrl_rms_norm_rows")
        assert np.array_equal(out.cpu().numpy(), want), f"clip {clip}"
        out = torch.full((k, dim), -12345.0, device=dev)
        _C.check(_C.lib().tsrl_rms_norm_rows(_C.ptr(xt), _C.ptr(mk), k, dim, _C.ptr(mt),
                                             _C.ptr(vt), float(eps), clip, _C.ptr(out),
                                             _C.stream_ptr(dev)), "tsrl_rms_norm_rows")
        o = out.cpu().numpy()
        assert np.array_equal(o[mask], want[mask]), f"selected rows, clip {clip}"
        assert (o[~mask] == F32(-12345.0)).all(), f"unselected rows keep the sentinel, clip {clip}"


# -----------------------------------------------------------------------------------------
# the producers: the synthetic env's partials
# -----------------------------------------------------------------------------------------
def _sums(rows):
    r = rows.astype(LD)
    return np.stack([r.sum(0), (r * r).sum(0)], axis=-1)


def _partials_equal_rows(p, rows, nblk, what):
    """Block-summed partials against the f64 column sums of the rows, relative nblk * 2^-53
    (the env's values are multiples of 2^-23 in [-1, 1): its block sums are exact in f64)."""
    got = p.astype(LD).sum(0)
    want = _sums(rows)
    assert np.isfinite(p).all(), what
    assert (np.abs(got - want) <= nblk * LD(2) ** -53 * np.abs(want)).all(), what


@pytest.mark.parametrize("k", [1, 15, 16, 17, 4096])
@pytest.mark.parametrize("dim", [5, 8, 376])
def test_env_partials_describe_the_rows_written(dev, k, dim):
    """The partials the env kernels hand to merge / merge2 are the column sums of the rows they
    wrote: reset (all rows, and a mask), step, and step + reset with blk_done counting the
    finished rows per 16-row block and the reset partials covering exactly those rows."""
    from tianshou_amd.env import SyntheticVectorEnv
    rng = np.random.default_rng(900 + k + dim)
    env = SyntheticVectorEnv(k, (dim,), 2, ep_len=3, seed=7, device=dev)
    nblk = env.nblk_for(k)
    assert nblk == (k + ROWS - 1) // ROWS

    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, float("nan"), dtype=dtype, device=dev)

    obs, part = nan(k, dim), nan(nblk, dim, 2, dtype=torch.float64)
    env._reset_raw(None, None, k, obs, part)
    _partials_equal_rows(part.cpu().numpy(), obs.cpu().numpy(), nblk, "reset of every row")

    rew = torch.empty(k, dtype=torch.float64, device=dev)
    term, trunc, done = (torch.zeros(k, dtype=torch.uint8, device=dev) for _ in range(3))
    obs, part = nan(k, dim), nan(nblk, dim, 2, dtype=torch.float64)
    env._step_raw(None, k, obs, rew, term, trunc, part)
    _partials_equal_rows(part.cpu().numpy(), obs.cpu().numpy(), nblk, "step")
    fin = (term | trunc).cpu().numpy().astype(bool)

    # reset of the finished rows of that step by mask (none finished: zero partials)
    robs, part = nan(k, dim), nan(nblk, dim, 2, dtype=torch.float64)
    env._reset_raw(None, torch.as_tensor(fin.astype(np.uint8), device=dev), k, robs, part)
    r = robs.cpu().numpy()
    assert np.isnan(r[~fin]).all() and np.isfinite(r[fin]).all()
    _partials_equal_rows(part.cpu().numpy(), r[fin], nblk, "masked reset")

    seen = 0
    for step in range(3):
        obs, robs = nan(k, dim), nan(k, dim)
        p1, p2 = nan(nblk, dim, 2, dtype=torch.float64), nan(nblk, dim, 2, dtype=torch.float64)
        bd = nan(nblk, dtype=torch.float64)
        env._step_reset_raw(k, obs, robs, rew, term, trunc, done, p1, p2, bd)
        dn = done.cpu().numpy().astype(bool)
        assert np.array_equal(dn, (term | trunc).cpu().numpy().astype(bool))
        _partials_equal_rows(p1.cpu().numpy(), obs.cpu().numpy(), nblk, f"step+reset {step}")
        per_blk = np.add.reduceat(dn.astype(np.int64), np.arange(0, k, ROWS))
        assert np.array_equal(bd.cpu().numpy(), per_blk.astype(np.float64)), "blk_done"
        r = robs.cpu().numpy()
        assert np.isfinite(r[dn]).all()
        live = p2.cpu().numpy()[per_blk > 0]
        _partials_equal_rows(live, r[dn], nblk, f"reset partials {step}")
        seen += int(dn.sum())
    assert seen == k  # ep_len 3: every env finished once in three steps
