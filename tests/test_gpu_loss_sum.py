"""The batch reduction that the off-policy loss kernels share (csrc/loss_sum.h), bit for bit.

The documented order is restated here in NumPy f64: the per-row terms padded with +0.0 to whole
workgroups of 256, each wave of 64 summed by the xor butterfly (offsets 32 ... 1) and read at
lane 0, the four waves added in wave order, the workgroups in block order, then the finish
(MeanLosses: loss[k] = sign * f32(s[k] / n), total = sign * f32(sum of the f64 quotients);
ActorAlphaLosses: loss[0] = f32(s[0] / b), m = s[1] / b, loss[1] = f32(-log_alpha * m),
g_log_alpha = f32(-m)).  f64 addition and division are IEEE-exact on both sides, so the losses
must agree in every bit: the tolerance is zero.

Only kernels whose per-row term is plain f32 arithmetic, which NumPy reproduces exactly on the
host, are held to this: tsrl_q_mse_fwd_bwd, tsrl_neg_mean_fwd_bwd, tsrl_dqn_td_fwd_bwd,
tsrl_dsac_q_loss_fwd_bwd, tsrl_redq_q_loss_fwd_bwd and tsrl_sac_actor_loss_fwd_bwd.
tsrl_dsac_actor_loss_fwd_bwd is left out: its row terms go through f64 exp and log on the
device, which the host's libm need not match in the last bit (tests/test_gpu_dsac.py holds it
to its f64 restatement at rtol 1e-5); tsrl_redq_actor_loss_fwd_bwd finishes with the functor of
the SAC actor loss.  b covers one lane, a whole wave, a wave and a lane, a whole workgroup (the
in-kernel finish), a workgroup and a lane, and four workgroups (the fold)."""
import numpy as np
import pytest
import torch

from tianshou_amd.policy.ddpg import neg_mean_loss, q_mse_loss
from tianshou_amd.policy.discrete_sac import dsac_q_loss
from tianshou_amd.policy.dqn import _DQNLoss
from tianshou_amd.policy.redq import redq_q_loss
from tianshou_amd.policy.sac import sac_actor_loss

gpu = pytest.mark.gpu  # the restatement's own test below runs on the host

BS = (1, 64, 65, 256, 257, 1000)
TPB, WAVE = 256, 64
F32, F64 = np.float32, np.float64


def ordered_sum(terms: np.ndarray) -> np.float64:
    """The f64 sum of ``terms`` [b] in the kernels' order."""
    assert terms.dtype == F64 and terms.ndim == 1
    nblk = -(-len(terms) // TPB)
    v = np.zeros(nblk * TPB, dtype=F64)
    v[:len(terms)] = terms
    v = v.reshape(nblk, TPB // WAVE, WAVE)
    lane = np.arange(WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ off]
    waves = v[..., 0]
    blocks = np.zeros(nblk, dtype=F64)
    for w in range(TPB // WAVE):
        blocks = blocks + waves[:, w]
    s = F64(0.0)
    for x in blocks:
        s = s + x
    return s


def mean_losses(sums, n, sign=1.0):
    """MeanLosses: (loss [len(sums)] f32, total f32)."""
    quot = [F64(s) / F64(n) for s in sums]
    tot = F64(0.0)
    for q in quot:
        tot = tot + q
    return np.array([F32(sign) * F32(q) for q in quot], dtype=F32), F32(sign) * F32(tot)


def actor_alpha_losses(s0, s1, b, log_alpha):
    """ActorAlphaLosses with sign0 = +1: (loss [1 or 2] f32, g_log_alpha f32 or None)."""
    loss = [F32(F64(s0) / F64(b))]
    if log_alpha is None:
        return np.array(loss, dtype=F32), None
    m = F64(s1) / F64(b)
    loss.append(F32(-F64(F32(log_alpha)) * m))
    return np.array(loss, dtype=F32), F32(-m)


def min_nan(a, c):
    return np.where(a != a, a, np.where(c != c, c, np.where(c < a, c, a)))


def test_ordered_sum_is_the_documented_order():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1000) * 2.0 ** rng.integers(-30, 30, 1000)
    s = ordered_sum(x)
    assert abs(s - np.sum(x)) <= 1e-12 * np.abs(x).sum()
    assert ordered_sum(np.array([3.0])) == 3.0
    # lane 0's butterfly pairs (0, 32) first: 1 + 2^-53 rounds to 1, twice
    y = np.zeros(64)
    y[0], y[32], y[16] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert ordered_sum(y) == 1.0
    # (16, 48) pair up to 2^-52 before they meet lane 0's 1; in index order the sum stays 1
    y[48] = 2.0 ** -53
    assert ordered_sum(y) == 1.0 + 2.0 ** -52


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.float32)


def _bits(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).reshape(-1).view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and np.array_equal(g, w), (what, g, w)


@gpu
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("critics", (1, 2))
@pytest.mark.parametrize("b", BS)
def test_q_mse_loss_bits(dev, b, critics, weighted):
    gen = torch.Generator().manual_seed(100 * b + 10 * critics + weighted)
    qs = [_randn(gen, b, scale=3.0) for _ in range(critics)]
    ret = _randn(gen, b, scale=3.0)
    w = torch.rand(b, generator=gen) + 0.5 if weighted else None
    total, loss, _ = q_mse_loss([q.to(dev) for q in qs], ret.to(dev),
                                None if w is None else w.to(dev))
    wn = np.ones(b, dtype=F32) if w is None else w.numpy()
    sums = []
    for q in qs:
        td = q.numpy() - ret.numpy()
        sums.append(ordered_sum((td * td * wn).astype(F64)))
    want, want_total = mean_losses(sums, b)
    _same_bits(loss, want, "loss")
    _same_bits(total, want_total, "total")


@gpu
@pytest.mark.parametrize("b", BS)
def test_neg_mean_loss_bits(dev, b):
    gen = torch.Generator().manual_seed(b)
    q = _randn(gen, b, 1, scale=5.0)
    loss = neg_mean_loss(q.to(dev))
    want, _ = mean_losses([ordered_sum(q.numpy().reshape(-1).astype(F64))], b, sign=-1.0)
    _same_bits(loss, want, "loss")


@gpu
@pytest.mark.parametrize("huber", (False, True))
@pytest.mark.parametrize("b", BS)
def test_dqn_td_loss_bits(dev, b, huber):
    A = 5
    gen = torch.Generator().manual_seed(2 * b + huber)
    q = _randn(gen, b, A, scale=2.0)  # |td| on both sides of the Huber knee
    ret = _randn(gen, b, scale=2.0)
    act = torch.randint(0, A, (b,), generator=gen)
    w = None if huber else torch.rand(b, generator=gen) + 0.5
    loss, _ = _DQNLoss.apply(q.to(dev), (act.to(dev), ret.to(dev),
                                         None if w is None else w.to(dev), huber, None, None))
    td = ret.numpy() - q.numpy()[np.arange(b), act.numpy()]
    if huber:
        ax = np.abs(td)
        term = np.where(ax < F32(1.0), F32(0.5) * td * td, ax - F32(0.5))
    else:
        term = td * td * w.numpy()
    assert term.dtype == F32
    want, _ = mean_losses([ordered_sum(term.astype(F64))], b)
    _same_bits(loss, want, "loss")


@gpu
@pytest.mark.parametrize("b", BS)
def test_dsac_q_loss_bits(dev, b):
    A = 6
    gen = torch.Generator().manual_seed(b)
    q1, q2 = _randn(gen, b, A, scale=2.0), _randn(gen, b, A, scale=2.0)
    ret = _randn(gen, b, scale=2.0)
    act = torch.randint(0, A, (b,), generator=gen)
    w = torch.rand(b, generator=gen) + 0.5
    total, loss, _ = dsac_q_loss(q1.to(dev), q2.to(dev), act.to(dev), ret.to(dev), w.to(dev))
    sums = []
    for q in (q1, q2):
        td = q.numpy()[np.arange(b), act.numpy()] - ret.numpy()
        sums.append(ordered_sum((td * td * w.numpy()).astype(F64)))
    want, want_total = mean_losses(sums, b)
    _same_bits(loss, want, "loss")
    _same_bits(total, want_total, "total")


@gpu
@pytest.mark.parametrize("b", BS)
def test_redq_q_loss_bits(dev, b):
    E = 3
    gen = torch.Generator().manual_seed(b)
    q = _randn(gen, E, b, scale=2.0)
    ret = _randn(gen, b, scale=2.0)
    w = torch.rand(b, generator=gen) + 0.5
    _, loss, _ = redq_q_loss(q.to(dev), ret.to(dev), w.to(dev))
    term = np.zeros(b, dtype=F64)
    for e in range(E):  # a column's members first, in f64 in index order
        td = q.numpy()[e] - ret.numpy()
        term = term + (td * td * w.numpy()).astype(F64)
    want, _ = mean_losses([ordered_sum(term)], float(E) * float(b))
    _same_bits(loss, want, "loss")


@gpu
@pytest.mark.parametrize("auto", (False, True))
@pytest.mark.parametrize("b", BS)
def test_sac_actor_loss_bits(dev, b, auto):
    gen = torch.Generator().manual_seed(2 * b + auto)
    q1, q2 = _randn(gen, b, scale=3.0), _randn(gen, b, scale=3.0)
    if b > 1:
        q2[1] = q1[1]  # a tie
    lp = _randn(gen, b, scale=4.0)
    alpha = torch.tensor([0.2371], dtype=torch.float32)
    log_alpha = torch.tensor([-1.4393], dtype=torch.float32) if auto else None
    target_entropy = -6.3
    _, loss, g_la = sac_actor_loss(q1.to(dev), q2.to(dev), lp.to(dev), alpha.to(dev),
                                   None if log_alpha is None else log_alpha.to(dev),
                                   target_entropy)
    p = alpha.numpy()[0] * lp.numpy()
    t0 = p - min_nan(q1.numpy(), q2.numpy())
    t1 = lp.numpy() + F32(target_entropy)
    assert p.dtype == t0.dtype == t1.dtype == F32
    want, want_g = actor_alpha_losses(ordered_sum(t0.astype(F64)), ordered_sum(t1.astype(F64)),
                                      b, None if log_alpha is None else log_alpha.numpy()[0])
    _same_bits(loss, want, "loss")
    if auto:
        _same_bits(g_la, want_g, "g_log_alpha")
