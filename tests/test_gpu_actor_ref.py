"""The collector's Gaussian policy step -- csrc/policy.hip (tsrl_gauss_policy_act[_rng]) and the
actor phase of the one-launch collect step (csrc/collect.hip) -- against references that share
no code with either kernel: oracle/actor_ref.py (numpy f64 actor, the counter-based noise
restated from its integer hash, map_action) and np.tanh in f64.  tests/test_actor_ref.py keeps
those references honest on the CPU and shows the headroom of every tolerance used here.

What is anchored:
  a. tanh_nb (csrc/tsrl_common.h) evaluated directly on the device, in ulp of f64 tanh;
  b. the noise stream cell by cell: row r, action a, step s gets counter_normal2(seed, s, r,
     a / 2) in both kernels, eager and replayed from a graph;
  c. policy.hip's actor against the f64 actor at shape edges, padded pitches, guard words,
     FlatAdam-bound parameters, and its refusals;
  d. map_action bit for bit (clip / scaling) and within tanh_nb's bound (tanh);
  e. collect.hip's actor against the f64 actor on the rows the collector stored.

Zero weights and biases with log_std = 0 make act = eps * 1 + 0 = eps exactly, which turns the
policy kernel into a probe: act_remap is then map_action of a chosen f32 (a, d), and act is the
raw device noise (b).

Every measured figure in the docstrings below was taken on an MI355X (gfx950).
"""
import numpy as np
import pytest
import torch

from oracle import actor_ref
from tests.actor_common import BOUND_CASE, SHAPE_CASES, layer_arrays, make_actor

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC
SENTINEL = -12345.0
GUARD = 64
# tanh_nb against f64 tanh over normal-range inputs: the maximum measured on the device (1.548
# ulp32, test_tanh_nb_against_f64) rounded up to the next half ulp
TANH_NB_ULP = 2.0
# the device's logf / sincospif / sqrtf may differ from the host libm's: 4 x the 2.2-2.3 ulp the
# f32 restatement of the formulas has against f64 (test_actor_ref.py), in ulp32 of max(|z|, 1)
NOISE_ULP = 9.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


class _Kernel:
    """tsrl_gauss_policy_act[_rng] on one actor, outputs behind guard words."""

    def __init__(self, actor, dev):
        from tianshou_amd.policy.fused_act import FusedGaussAct, match_actor
        self.dev = dev
        self.layers = match_actor(actor)
        assert self.layers is not None
        self.fa = FusedGaussAct(self.layers)
        self.fa.pack()
        self.D, self.A = self.layers["D"], self.layers["A"]

    def arrays(self):
        return layer_arrays(self.layers)

    def run(self, obs, n, eps=None, bound=None, low=None, high=None, ldx=None, act_dim=None,
            obs_ptr=None, rng=None):
        """-> (rc, act [n, A], act_remap [n, A]) as numpy f32; asserts the guards untouched.
        ``rng`` = (seed, ctr_in, ctr_out) selects tsrl_gauss_policy_act_rng."""
        from tianshou_amd import _C
        from tianshou_amd.policy.fused_act import _BOUND
        L, Ly = _C.lib(), self.layers
        A = self.A if act_dim is None else act_dim
        out = torch.full((2, n * self.A + GUARD), SENTINEL, device=self.dev)
        head = (obs.data_ptr() if obs_ptr is None else obs_ptr,
                obs.stride(0) if ldx is None else ldx, n, self.D, _C.ptr(self.fa.packed),
                _C.ptr(Ly["w1"].bias.detach()), _C.ptr(Ly["w2"].weight.detach()),
                _C.ptr(Ly["w2"].bias.detach()), _C.ptr(Ly["w3"].weight.detach()),
                _C.ptr(Ly["w3"].bias.detach()), _C.ptr(Ly["sigma"].detach()), A)
        tail = (_BOUND[bound], _C.ptr(low), _C.ptr(high), out[0].data_ptr(), out[1].data_ptr(),
                _C.stream_ptr(self.dev))
        if rng is None:
            rc = L.tsrl_gauss_policy_act(*head, _C.ptr(eps), *tail)
        else:
            seed, cin, cout = rng
            rc = L.tsrl_gauss_policy_act_rng(*head, seed, _C.ptr(cin), _C.ptr(cout), *tail)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert (o[:, n * self.A:] == SENTINEL).all(), "guard words after n * A were written"
        return rc, o[0, :n * self.A].reshape(n, self.A), o[1, :n * self.A].reshape(n, self.A)


def _zero_kernel(D, A, dev):
    actor, _ = make_actor(D, A, dev, 1)
    with torch.no_grad():
        for p in actor.parameters():
            p.zero_()
    return _Kernel(actor, dev), actor


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def probe(dev):
    """Zero actor of A = 32 on 4096 rows: 131072 chosen f32 per launch through the eps operand."""
    k, _ = _zero_kernel(4, 32, dev)
    obs = torch.zeros(4096, 4, device=dev)

    def run(x, bound, low=None, high=None):
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        acts, remaps = [], []
        for i in range(0, x.size, 131072):
            chunk = np.ones(131072, np.float32)
            m = min(131072, x.size - i)
            chunk[:m] = x[i:i + m]
            eps = torch.from_numpy(chunk.reshape(4096, 32)).to(dev)
            rc, act, remap = k.run(obs, 4096, eps=eps, bound=bound, low=low, high=high)
            assert rc == 0
            acts.append(act.reshape(-1)[:m])
            remaps.append(remap.reshape(-1)[:m])
        return np.concatenate(acts), np.concatenate(remaps)
    return run


# ---- a. tanh_nb ------------------------------------------------------------------------------
def _tanh_inputs():
    f = np.float32
    rng = np.random.default_rng(0)
    parts = {}
    seam = np.arange(-4096, 4097, dtype=np.int32) + _bits(f(0.625))
    seam = seam.view(np.float32)
    parts["seam"] = np.concatenate([seam, -seam])
    e = rng.integers(-126, 7, 1 << 18)                       # 2^-126 <= |x| < 2^7
    mant = 1.0 + rng.integers(0, 1 << 23, 1 << 18) * 2.0 ** -23
    sign = np.where(rng.integers(0, 2, 1 << 18) == 0, 1.0, -1.0)
    parts["log"] = (sign * np.ldexp(mant, e)).astype(f)
    parts["uniform"] = rng.uniform(-10.0, 10.0, 1 << 18).astype(f)
    d = np.array([2.0 ** -126, 9.0, 9.02, 44.0, 45.0, 88.0, 89.0, np.finfo(f).max, np.inf], f)
    parts["directed"] = np.concatenate([d, -d, np.array([np.nan], f)])
    den = rng.integers(1, 1 << 23, 512).astype(np.int32).view(np.float32)
    parts["denormal"] = np.concatenate([den, -den])
    return parts


def test_tanh_nb_against_f64(probe):
    """tanh_nb on 541717 inputs (the 0.625 seam +-4096 ulp both signs, 2^18 log-uniform from
    2^-126 to 2^7, 2^18 uniform in [-10, 10], directed values, 1024 denormals) against np.tanh
    in f64.

    Measured (MI355X): maximum over the normal-range inputs 1.548 ulp32, at x = 0.62514120 just
    above the seam (seam set 1.548, log-uniform 1.478 at 0.7279, uniform 1.489 at 0.6353,
    directed 0.489 at 9.0): the device's v_exp_f32 / v_rcp_f32 stay inside the 1.6 ulp that
    tsrl_common.h had from an emulation with correctly rounded exp2 / rcp.  Denormal inputs
    come back bit-identical (|y - x| = 0), and a NaN eps reaches act with its bits (0x7fc00000).
    The asserted bound TANH_NB_ULP = 2.0 is the measured maximum rounded up to the next half
    ulp; the seam moved to 0.5 measures 2.29 and fails it."""
    parts = _tanh_inputs()
    names = list(parts)
    x = np.concatenate([parts[k] for k in names])
    assert x.size == 2 * 8193 + 2 * (1 << 18) + 19 + 1024
    act, y = probe(x, "tanh")
    normal = np.isfinite(x) & (np.abs(x) >= 2.0 ** -126)
    assert (x != 0).all()
    den = ~normal & np.isfinite(x)
    print("NaN eps -> act bits", [hex(int(b) & 0xFFFFFFFF) for b in _bits(act)[np.isnan(x)]],
          "from", [hex(int(b) & 0xFFFFFFFF) for b in _bits(x)[np.isnan(x)]])
    print("denormal eps -> act bit-identical:", np.array_equal(_bits(act)[den], _bits(x)[den]))
    # the probe: act == eps bit for bit (finite non-zero -- denormals too --, infinite, NaN)
    assert np.array_equal(_bits(act), _bits(x))
    x64 = x.astype(np.float64)
    want = np.tanh(x64)
    err = actor_ref.ulp_err32(y, want)
    o = 0
    for k in names:
        m = slice(o, o + parts[k].size)
        o += parts[k].size
        nm = normal[m]
        if nm.any():
            i = np.flatnonzero(nm)[np.argmax(err[m][nm])]
            print("tanh_nb %-9s max %.4f ulp32 at x = %r" % (k, err[m][i], float(x[m][i])))
    worst = err[normal].max()
    print("tanh_nb normal-range max %.4f ulp32 (asserted %.1f)" % (worst, TANH_NB_ULP))
    # exact properties, every input
    fin = ~np.isnan(x)
    assert np.isnan(y[~fin]).all()
    assert not np.isnan(y[fin]).any()
    assert (np.abs(y[fin]) <= 1.0).all()
    big = fin & (np.abs(x) >= 45.0)
    assert np.array_equal(y[big], np.sign(x[big]).astype(np.float32))
    assert np.array_equal(np.signbit(y[fin]), np.signbit(x[fin]))
    assert (y[normal] != 0).all()
    # denormals: tanh(x) = x (1 - x^2 / 3 ...) is x to far below the f32 grid
    dd = np.abs(y[den].astype(np.float64) - x64[den])
    print("tanh_nb denormal inputs: bit-identical %s, max |y - x| = %.3e"
          % (np.array_equal(_bits(y)[den], _bits(x)[den]), dd.max()))
    assert (dd <= 2.0 ** -126).all()
    assert worst <= TANH_NB_ULP


# ---- b. the noise stream ---------------------------------------------------------------------
def _noise_err(act, z):
    """max |act - z| in ulp32 of max(|z|, 1)."""
    unit = np.spacing(np.maximum(np.abs(z), 1.0).astype(np.float32)).astype(np.float64)
    return (np.abs(act.astype(np.float64) - z) / unit).max()


@pytest.mark.parametrize("A", [1, 5, 32])
def test_policy_noise_is_counter_normal_cell_by_cell(dev, A):
    """tsrl_gauss_policy_act_rng with zero weights: act[r, a] of the call at step s is
    counter_normal(seed, s, r, a) for s = 7, 8, 9 through a ping-pong counter pair, three
    workgroups (n = 70: the last ragged).  Measured (MI355X): at most 1.52 (A = 1), 1.54 (A = 5),
    1.81 (A = 32) ulp32 of max(|z|, 1) (asserted 9; an indexing mistake is an O(1) error, millions of ulp).  Then with log_std and b3 set: act == z * expf(log_std) + b3 in
    two f32 roundings, bit for bit, z the kernel's own raw noise and expf(log_std) the
    device's (read back through an eps = 1 launch)."""
    n, D = 70, 8
    k, actor = _zero_kernel(D, A, dev)
    obs = torch.randn(n, D, device=dev)
    ctr = torch.tensor([7, -1], dtype=torch.int64, device=dev)
    raw = []
    for i in range(3):
        p = i % 2
        rc, act, remap = k.run(obs, n, rng=(SEED, ctr[p:p + 1], ctr[1 - p:2 - p]))
        assert rc == 0
        assert int(ctr[1 - p].item()) == 8 + i and int(ctr[p].item()) == 7 + i
        z =actor_ref.counter_normal(SEED, 7 + i, np.arange(n), A)
        e = _noise_err(act, z)
        print("A %d step %d: %.3f ulp32 of max(|z|, 1)" % (A, 7 + i, e))
        assert e <= NOISE_ULP
        assert np.array_equal(_bits(act), _bits(remap))  # no bound, no scaling
        raw.append(act)
    assert not np.array_equal(raw[0], raw[1]) and not np.array_equal(raw[1], raw[2])
    # sigma and b3: two roundings on top of the same noise
    g = torch.Generator().manual_seed(A)
    with torch.no_grad():
        actor.sigma_param.copy_((0.7 * torch.randn(A, generator=g)).view_as(actor.sigma_param))
    # the device's expf(log_std): eps = 1, mu = b3 = 0 -> act = 1 * sigma + 0
    rc, sigma, _ = k.run(obs, n, eps=torch.ones(n, A, device=dev))
    assert rc == 0
    want_sigma = np.exp(k.arrays()[6])
    assert (actor_ref.ulp_err32(sigma, np.broadcast_to(want_sigma, sigma.shape)) <= 2.0).all()
    with torch.no_grad():
        k.layers["w3"].bias.copy_(torch.randn(A, generator=g))
    b3 = k.layers["w3"].bias.detach().cpu().numpy()
    ctr = torch.tensor([7, -1], dtype=torch.int64, device=dev)
    rc, act, _ = k.run(obs, n, rng=(SEED, ctr[0:1], ctr[1:2]))
    assert rc == 0 and int(ctr[1].item()) == 8
    want = (raw[0] * sigma).astype(np.float32) + b3[None, :].astype(np.float32)
    assert want.dtype == np.float32
    assert np.array_equal(_bits(act), _bits(want))


def _collector(dev, E, D, A, T, graph_steps, zero, act_coef=0.0, ep_len=2, collects=1):
    from tianshou_amd.data import Collector, VectorReplayBuffer
    from tianshou_amd.env import Box, SyntheticVectorEnv, VectorEnvNormObs
    from tianshou_amd.policy import PPOPolicy
    from tianshou_amd.utils.models import fixed_std_normal, get_actor_critic, init_and_get_optim
    torch.manual_seed(D + A)
    actor, critic = get_actor_critic((D,), (64, 64), (A,), dev)
    optim = init_and_get_optim(actor.to(dev), critic.to(dev), 3e-4)
    with torch.no_grad():
        for p in actor.parameters():
            if zero:
                p.zero_()
            else:
                p.add_(0.05 * torch.randn_like(p))
    pol = PPOPolicy(actor, critic, optim, fixed_std_normal, action_space=Box(-2.0, 3.0, (A,)),
                    action_bound_method="clip").to(dev)
    env = VectorEnvNormObs(SyntheticVectorEnv(E, (D,), A, ep_len=ep_len, seed=5, device=dev,
                                              act_coef=act_coef))
    buf = VectorReplayBuffer(E * T * collects, E, device=dev)
    c = Collector(pol, env, buf)
    c.use_fused_step = True
    c.graph_steps = graph_steps
    return c, pol, buf


def _noise_ctr(c):
    """The noise step counter the next collect step reads."""
    return int(c._scratch["step_ctr"][c._parity, 1].item())


def _stored(buf, E, name):
    """buffer rows as [env, step, ...] (VectorReplayBuffer: one ring of equal size per env)."""
    x = getattr(buf._meta, name).detach().cpu().numpy()
    return x.reshape((E, x.shape[0] // E) + x.shape[1:])


@pytest.mark.parametrize("graph_steps", [0, 4])
def test_collect_noise_is_counter_normal_cell_by_cell(dev, graph_steps):
    """The fused collect step with zero weights: the stored act[t, e] is counter_normal(seed,
    ctr0 + t, e, a), eager (graph_steps 0) and with steps 1-4 of each collect replayed from a
    captured graph (graph_steps 4); E = 17 is one full 16-row tile and a 1-row tile.  A second
    collect continues the counter.  Measured (MI355X): at most 1.43 ulp32 of max(|z|, 1), the
    same eager and replayed."""
    E, D, A, T = 17, 5, 3, 6
    c, pol, buf = _collector(dev, E, D, A, T, graph_steps, zero=True, collects=2)
    ctr0 = _noise_ctr(c)
    c.collect(n_step=E * T)
    assert c._step_on
    seed = pol._fused_act._seed
    assert _noise_ctr(c) == ctr0 + T
    c.collect(n_step=E * T)
    assert c._step_on and _noise_ctr(c) == ctr0 + 2 * T
    assert bool(c._graphs) == bool(graph_steps)  # steps were (not) replayed from a captured graph
    assert pol._fused_act._seed == seed
    torch.cuda.synchronize()
    act = _stored(buf, E, "act")
    assert act.shape == (E, 2 * T, A)
    worst = 0.0
    for t in range(2 * T):
        z = actor_ref.counter_normal(seed, ctr0 + t, np.arange(E), A)
        e = _noise_err(act[:, t], z)
        worst = max(worst, e)
        assert e <= NOISE_ULP, (t, e)
    print("collect noise, graph_steps %d: %.3f ulp32 of max(|z|, 1)" % (graph_steps, worst))
    rows = act.transpose(1, 0, 2).reshape(2 * T * E, A)
    assert np.unique(rows, axis=0).shape[0] == rows.shape[0]


# ---- c. policy.hip's actor at shape edges ----------------------------------------------------
def _case_inputs(D, A, n):
    g = torch.Generator().manual_seed(1000 * D + A)
    obs = torch.randn(n, D, generator=g)
    eps = torch.randn(n, A, generator=g)
    low = -1.0 - torch.rand(A, generator=g)
    high = 1.0 + 2 * torch.rand(A, generator=g)
    return obs, eps, low, high


def _check_against_f64(k, obs, eps, low, high, n, dev, label):
    rc, act, remap = k.run(obs.to(dev), n, eps=eps.to(dev), bound="clip", low=low.to(dev),
                           high=high.to(dev))
    assert rc == 0
    want, want_remap = actor_ref.gauss_act_ref(obs.numpy(), *k.arrays(), eps.numpy(), "clip",
                                               low.numpy(), high.numpy())
    share = max((np.abs(act - want) / (1e-5 + 1e-5 * np.abs(want))).max(),
                (np.abs(remap - want_remap) / (1e-5 + 1e-5 * np.abs(want_remap))).max())
    print("%s: max |act - f64| %.3e, %.4f of the tolerance"
          % (label, np.abs(act - want).max(), share))
    assert not np.isnan(act).any() and not np.isnan(remap).any()
    np.testing.assert_allclose(act, want, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(remap, want_remap, rtol=1e-5, atol=1e-5)
    return act, remap


@pytest.mark.parametrize("D,A,n", SHAPE_CASES)
def test_policy_actor_against_f64(dev, D, A, n):
    """tsrl_gauss_policy_act with explicit eps against gauss_act_ref, rtol = atol = 1e-5 (the
    kernel's own tolerance; a correct f32 evaluation stays under 0.05 of it,
    test_actor_ref.py).  The three variant shapes run again on a padded pitch (ldx = D + 4:
    the float4 row path stays where D % 4 == 0) and on ldx = D + 1 (the scalar row path even
    for D % 4 == 0), pads and two rows past n filled with NaN: bit-identical outputs, no NaN.

    Measured (MI355X), max |act - f64| and its share of the tolerance:
        D     A    n    max |act - f64|   share of tolerance
        1     1    1    1.28e-07          0.006
        3     2    31   1.59e-07          0.016
        5     2    33   7.19e-08          0.025
        16    31   32   1.34e-07          0.021
        17    6    70   1.51e-07          0.018
        33    32   70   2.37e-07          0.033
        48    17   70   2.14e-07          0.024
        376   17   70   2.20e-07          0.033
        1000  32   70   4.18e-07          0.058
    """
    actor, _ = make_actor(D, A, dev, D + A)
    k = _Kernel(actor, dev)
    obs, eps, low, high = _case_inputs(D, A, n)
    act, remap = _check_against_f64(k, obs, eps, low, high, n, dev, "D %d A %d n %d" % (D, A, n))
    if (D, A, n) not in ((16, 31, 32), (376, 17, 70), (17, 6, 70)):
        return
    for ldx in (D + 4, D + 1):
        pad = torch.full((n + 2, ldx), float("nan"))
        pad[:n, :D] = obs
        pad = pad.to(dev)
        rc, act2, remap2 = k.run(pad, n, eps=eps.to(dev), bound="clip", low=low.to(dev),
                                 high=high.to(dev), ldx=ldx)
        assert rc == 0
        assert not np.isnan(act2).any() and not np.isnan(remap2).any()
        assert np.array_equal(_bits(act2), _bits(act)), ldx
        assert np.array_equal(_bits(remap2), _bits(remap)), ldx


def test_policy_actor_on_flat_adam_storage(dev):
    """The production layout: after FusedActorCritic.bind_adam every parameter is a view into
    FlatAdam's flat buffer, back to back with no alignment padding, and the kernel reads w2 / w3
    as float4 without a host alignment check.  Here (D 24, A 17) the actor's sigma comes first,
    so w1 / w2 / w3 start 17 / 1617 / 5777 floats into the buffer, each 4 bytes past a 16-byte
    boundary: the float4 loads are misaligned and the device serves them (unaligned access mode).
    Measured (MI355X): max |act - f64| 1.83e-07, 0.031 of the tolerance."""
    from tianshou_amd.policy import fused_mlp
    from tianshou_amd.utils.net import ActorCritic
    D, A, n = BOUND_CASE
    actor, critic = make_actor(D, A, dev, D + A)
    ac = ActorCritic(actor, critic)
    opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
    fm = fused_mlp.FusedActorCritic(fused_mlp.match(actor, critic), ac.parameters())
    assert fm.bind_adam(opt) and fm.adam_bound(opt)
    k = _Kernel(actor, dev)
    flat = fm._adam["p"]
    for name in ("w1", "w2", "w3"):
        w = k.layers[name].weight
        assert flat.data_ptr() <= w.data_ptr() < flat.data_ptr() + 4 * flat.numel()
        print("%s at flat offset %d floats (address %% 16 = %d)"
              % (name, fm.flat_offset(w), w.data_ptr() % 16))
    obs, eps, low, high = _case_inputs(D, A, n)
    _check_against_f64(k, obs, eps, low, high, n, dev, "flat D %d A %d n %d" % (D, A, n))


def test_policy_act_refusals(dev):
    """Bad arguments return rc != 0 and launch nothing (outputs keep their preset)."""
    D, A, n = 8, 5, 40
    actor, _ = make_actor(D, A, dev, 3)
    k = _Kernel(actor, dev)
    obs = torch.randn(n + 1, D, device=dev)
    eps = torch.randn(n, A, device=dev)
    low, high = torch.full((A,), -1.0, device=dev), torch.full((A,), 1.0, device=dev)

    def refused(**kw):
        rc, act, remap = k.run(obs, n, eps=eps, bound="clip", **kw)
        return rc != 0 and (act == SENTINEL).all() and (remap == SENTINEL).all()
    rc, act, _ = k.run(obs, n, eps=eps, bound="clip", low=low, high=high)
    assert rc == 0 and not (act == SENTINEL).any()
    assert refused(act_dim=33)
    assert refused(act_dim=0)
    assert refused(ldx=D - 1)
    assert refused(low=low)
    assert refused(high=high)
    # rows read as float4 (D % 4 == 0, ldx % 4 == 0) from a base 4 bytes off a 16-byte boundary
    assert obs.data_ptr() % 16 == 0
    assert refused(obs_ptr=obs.data_ptr() + 4)
    ctr = torch.zeros(2, dtype=torch.int64, device=dev)
    rc, act, _ = k.run(obs, n, rng=(SEED, ctr[0:1], ctr[0:1]))  # counter in == out
    assert rc != 0 and (act == SENTINEL).all()


# ---- d. map_action ---------------------------------------------------------------------------
def _map_inputs():
    f = np.float32
    d = np.array([-np.inf, -1.0 - 2.0 ** -23, -1.0, -1.0 + 2.0 ** -24, 0.0, 1.0 - 2.0 ** -24, 1.0,
                  1.0 + 2.0 ** -23, np.inf, np.nan], f)
    assert d[1] < -1 and d[3] > -1 and d[5] < 1 and d[7] > 1  # all representable
    rng = np.random.default_rng(3)
    x = (1.5 * rng.standard_normal(4096 * 32)).astype(f)
    x[x == 0] = f(0.25)
    # the directed values in every action column (each column has its own low / high)
    for j in range(32):
        x.reshape(4096, 32)[100 + np.arange(d.size), j] = d
    return x, d


@pytest.mark.parametrize("bound", [None, "clip"])
@pytest.mark.parametrize("scale", [False, True])
def test_map_action_bit_exact(dev, probe, bound, scale):
    """act_remap == the numpy f32 evaluation of clamp (closed interval, NaN passes) then
    lo + (hi - lo) * (y + 1) / 2, every operation rounded, applied to the kernel's own act."""
    f = np.float32
    x, d = _map_inputs()
    rng = np.random.default_rng(4)
    lo = (-1.0 - rng.random(32)).astype(f)
    hi = (1.0 + 2.0 * rng.random(32)).astype(f)
    lohi = (torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev)) if scale else (None, None)
    act, remap = probe(x, bound, *lohi)
    nz = ~np.isnan(x) & (x != 0)
    assert np.array_equal(_bits(act)[nz], _bits(x)[nz])  # +0 * 1 + 0 = +0 too, -0 is not used
    assert np.isnan(act[np.isnan(x)]).all()
    y = act.reshape(4096, 32).copy()
    if bound == "clip":
        y = np.where(y < f(-1), f(-1), np.where(y > f(1), f(1), y))
    if scale:
        with np.errstate(invalid="ignore", over="ignore"):
            y = lo[None, :] + ((hi - lo)[None, :] * (y + f(1))) / f(2)
    assert y.dtype == f
    y = y.reshape(-1)
    nan = np.isnan(y)
    assert np.array_equal(nan, np.isnan(x))  # only NaN maps to NaN (inf - inf never arises)
    assert np.isnan(remap[nan]).all()
    assert np.array_equal(_bits(remap)[~nan], _bits(y)[~nan])
    if not scale:
        r = remap.reshape(4096, 32)[100:100 + d.size, 0]
        if bound == "clip":
            want = np.array([-1, -1, -1, d[3], 0, d[5], 1, 1, 1], f)
        else:
            want = d[:9]
        assert np.array_equal(_bits(r[:9]), _bits(want))


def test_map_action_tanh_scaled_within_bound(dev, probe):
    """tanh then scaling: within tanh_nb's measured bound carried through the affine map, and
    inside [low, high].  low / high are multiples of 1/8 with an exact difference: then
    (hi - lo) * (y + 1) / 2 <= hi - lo for |y| <= 1 by the monotonicity of each rounding, and
    lo + that <= hi (hi is representable), so containment is a property of a correct kernel.
    (For a low / high pair whose difference rounds up, lo + fl(hi - lo) may exceed hi by one
    ulp in torch's formula too.)"""
    f = np.float32
    x, d = _map_inputs()
    rng = np.random.default_rng(5)
    lo = (-rng.integers(1, 32, 32) / 8.0).astype(f)
    hi = (rng.integers(1, 48, 32) / 8.0).astype(f)
    act, remap = probe(x, "tanh", torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))
    ok = ~np.isnan(x)
    x64 = act.astype(np.float64).reshape(4096, 32)
    lo64, hi64 = lo.astype(np.float64)[None, :], hi.astype(np.float64)[None, :]
    t = np.tanh(x64)
    want = lo64 + (hi64 - lo64) * (t + 1.0) / 2.0
    with np.errstate(invalid="ignore"):
        ulp_t = np.spacing(np.abs(t).astype(f)).astype(np.float64)
    half = 0.5 * float(np.spacing(f(1.0)))                        # rounding of y + 1 in [1, 2]
    scale = (hi64 - lo64) / 2.0
    tol = (scale * (TANH_NB_ULP * ulp_t + half)                  # tanh_nb, y + 1
           + 0.5 * np.spacing((4.0 * scale).astype(f))           # the product, <= 2 (hi - lo)
           + 0.5 * np.spacing(np.maximum(-lo64, hi64).astype(f)))  # the final sum
    r = remap.reshape(4096, 32).astype(np.float64)
    ok = ok.reshape(4096, 32)
    assert np.isnan(remap[np.isnan(x)]).all()
    excess = (np.abs(r - want) / tol)[ok].max()
    print("tanh + scaling: %.3f of the propagated bound" % excess)
    assert excess <= 1.0
    assert (r[ok] >= np.broadcast_to(lo64, r.shape)[ok]).all()
    assert (r[ok] <= np.broadcast_to(hi64, r.shape)[ok]).all()


# ---- e. collect.hip's actor ------------------------------------------------------------------
@pytest.mark.parametrize("E,D,A,act_coef", [
    (17, 5, 1, 0.0),       # one full and one 1-row tile, D % 4 == 1, a single action
    (100, 17, 6, 0.0),     # config 2's width, 7 workgroups (the last of 4 rows)
    (33, 24, 32, 0.0),     # A = AMAX: both 16-action tiles of the mu head full
    (100, 376, 17, 0.0),   # the headline width
    (20, 512, 5, 0.0),     # D = KMAX
    (100, 17, 6, 0.05),    # the action-coupled env: the actor runs before the env phase
])
def test_collect_actor_against_f64(dev, E, D, A, act_coef):
    """The fused collect step, eager, T = 3 steps with resets in between (ep_len 2): every
    stored act row against exp(log_std) * counter_normal(seed, ctr0 + t, e, .) + mu64(stored
    obs row), rtol = atol = 1e-5.  The stored (normalised) obs row IS the actor's input:
    collect.hip phase A puts the live row into the LDS tile sX, and both the buffer's obs row
    and layer 1 read sX (no path stores anything else).

    Measured (MI355X), max |act - f64| and its share of the tolerance:
        E     D     A    act_coef   max |act - f64|   share of tolerance
        17    5     1    0          1.45e-07          0.007
        100   17    6    0          2.13e-07          0.015
        33    24    32   0          3.16e-07          0.016
        100   376   17   0          3.09e-07          0.018
        20    512   5    0          2.84e-07          0.021
        100   17    6    0.05       2.75e-07          0.014
    """
    from tianshou_amd.policy.fused_act import match_actor
    T = 3
    c, pol, buf = _collector(dev, E, D, A, T, 0, zero=False, act_coef=act_coef)
    ctr0 = _noise_ctr(c)
    c.collect(n_step=E * T)
    assert c._step_on and c._fused_act_on
    torch.cuda.synchronize()
    seed = pol._fused_act._seed
    arrs = layer_arrays(match_actor(pol.actor))
    obs, act = _stored(buf, E, "obs"), _stored(buf, E, "act")
    assert obs.shape == (E, T, D) and act.shape == (E, T, A)
    assert not np.array_equal(obs[:, 0], obs[:, 1])
    worst = share = 0.0
    for t in range(T):
        z = actor_ref.counter_normal(seed, ctr0 + t, np.arange(E), A)
        want, _ = actor_ref.gauss_act_ref(obs[:, t], *arrs, z, None)
        worst = max(worst, np.abs(act[:, t] - want).max())
        share = max(share, (np.abs(act[:, t] - want) / (1e-5 + 1e-5 * np.abs(want))).max())
    print("collect E %d D %d A %d coef %g: max |act - f64| %.3e, %.4f of the tolerance"
          % (E, D, A, act_coef, worst, share))
    for t in range(T):
        z = actor_ref.counter_normal(seed, ctr0 + t, np.arange(E), A)
        want, _ = actor_ref.gauss_act_ref(obs[:, t], *arrs, z, None)
        np.testing.assert_allclose(act[:, t], want, rtol=1e-5, atol=1e-5)
