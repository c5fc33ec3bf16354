"""ORACLE (test infrastructure only) -- NumPy f64 restatement of the collector's Gaussian policy
step: the counter-based exploration noise (csrc/noise.h ``counter_normal2``) and the actor +
sampling + ``map_action`` of csrc/policy.hip / the actor phase of csrc/collect.hip.

Only ``tests/`` may import this module.  Nothing here touches torch or a GPU: the integer part
of the noise is exact in ``uint64`` and everything after it is IEEE f64, so the HIP kernels are
compared with a reference that shares neither their noise header, nor ``tanh_nb``, nor their
summation order.

Spec of the noise (identical in policy.hip and collect.hip; both C entries hash the caller's
seed once with ``sm64`` before the launch):

* ``h = sm(sm(sm(seed) ^ step) ^ ((row << 5) | pair))``, ``sm`` = oracle/synth_env.py ``sm``.
* ``u1 = ((h >> 40) + 1) 2^-24`` in (0, 1], ``u2 = ((h >> 16) & 0xFFFFFF) 2^-24`` in [0, 1).
* ``r = sqrt(-2 ln u1)``; action 2 pair gets ``r cos(2 pi u2)``, action 2 pair + 1 gets
  ``r sin(2 pi u2)``.
"""
import numpy as np

from oracle.synth_env import sm


def _hash_uniforms(seed, step, rows, A):
    """u1 in (0, 1], u2 in [0, 1) as exact f64, shape [len(rows), ceil(A / 2)]."""
    rows = np.atleast_1d(np.asarray(rows)).astype(np.int64).astype(np.uint64)
    pairs = np.arange((A + 1) // 2, dtype=np.uint64)
    s = sm(sm(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
           ^ np.asarray(int(step), dtype=np.int64).astype(np.uint64))
    h = sm(s ^ ((rows[:, None] << np.uint64(5)) | pairs[None, :]))
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def _interleave(zc, zs, A):
    z = np.empty((zc.shape[0], 2 * zc.shape[1]), dtype=zc.dtype)
    z[:, 0::2] = zc
    z[:, 1::2] = zs
    return z[:, :A]


def counter_normal(seed, step, rows, A):
    """The standard normals ``counter_normal2`` defines for (seed, step, row, action):
    float64 [len(rows), A]."""
    u1, u2 = _hash_uniforms(seed, step, rows, A)
    r = np.sqrt(-2.0 * np.log(u1))
    th = 2.0 * np.pi * u2
    return _interleave(r * np.cos(th), r * np.sin(th), A)


def counter_normal_f32(seed, step, rows, A):
    """The same formulas with every operation rounded to f32, in the kernel's order:
    ``r = sqrtf(-2 logf(u1))`` in f32 arithmetic, ``sincospif(2 u2)`` as an f32-rounded sine and
    cosine of the exact angle (sincospi's argument ``2 u2`` is exact in f32 and its reduction is
    exact by definition, so no rounded ``pi * x`` enters), then the two f32 products.  What a
    correct f32 implementation computes up to its libm; float32 [len(rows), A]."""
    u1, u2 = _hash_uniforms(seed, step, rows, A)
    f = np.float32
    r = np.sqrt(f(-2.0) * np.log(u1.astype(f)))  # u1 exact in f32: a 24-bit integer times 2^-24
    th = 2.0 * np.pi * u2
    zc, zs = r * np.cos(th).astype(f), r * np.sin(th).astype(f)
    return _interleave(zc.astype(f), zs.astype(f), A)


def actor_mu(obs, W1, b1, W2, b2, W3, b3):
    """mu = Linear(64, A)(tanh(Linear(64, 64)(tanh(Linear(D, 64)(obs))))) in f64; weights in
    torch's [out, in] layout."""
    d = np.float64
    x = np.asarray(obs, d)
    h1 = np.tanh(x @ np.asarray(W1, d).T + np.asarray(b1, d))
    h2 = np.tanh(h1 @ np.asarray(W2, d).T + np.asarray(b2, d))
    return h2 @ np.asarray(W3, d).T + np.asarray(b3, d)


def map_action(act, bound, low=None, high=None):
    """policy/base.py map_action in f64: ``bound`` in (None, "clip", "tanh"), then the affine
    map of [-1, 1] onto [low, high] when both are given."""
    y = np.asarray(act, np.float64)
    if bound == "clip":
        y = np.clip(y, -1.0, 1.0)
    elif bound == "tanh":
        y = np.tanh(y)
    elif bound is not None:
        raise ValueError(f"unknown bound {bound!r}")
    if (low is None) != (high is None):
        raise ValueError("low and high come together")
    if low is not None:
        lo, hi = np.asarray(low, np.float64), np.asarray(high, np.float64)
        y = lo + (hi - lo) * (y + 1.0) / 2.0
    return y


def gauss_act_ref(obs, W1, b1, W2, b2, W3, b3, log_std, eps, bound, low=None, high=None):
    """(act, act_remap) of the fused Gaussian policy step in f64: ``act = eps exp(log_std) +
    mu`` (``eps`` None: the deterministic act = mu), ``act_remap = map_action(act)``."""
    mu = actor_mu(obs, W1, b1, W2, b2, W3, b3)
    act = mu
    if eps is not None:
        act = np.asarray(eps, np.float64) * np.exp(np.asarray(log_std, np.float64)) + mu
    return act, map_action(act, bound, low, high)


def ulp_err32(got_f32, want_f64):
    """|got - want| in units of the f32 spacing at ``want`` (NaN where either is NaN; inf where
    an infinity is missed)."""
    got = np.asarray(got_f32, np.float32).astype(np.float64)
    want = np.asarray(want_f64, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        same_inf = np.isinf(want) & (got == want)
        return np.where(same_inf, 0.0, np.abs(got - want) / sp)
