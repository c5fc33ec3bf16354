"""The kernels of csrc/noisy.hip through the C ABI and through utils/net.py's NoisyLinear and
dueling_combine.

tsrl_noisy_eps, tsrl_noisy_weights, tsrl_noisy_grads: exact equality with the reference's torch
formulation on the device (discrete.py:361-374 and autograd's gradients of it) -- every product
and sum is rounded once in both, the square root is correctly rounded in both -- with canaries
around every output, at element counts and (in, out) shapes on both sides of the wave, of the
256-thread workgroup and of the 16-byte vector path, each layer alone and all of them as one
table over consecutive views of one flat buffer (so several layers start 4-byte aligned only,
the vectorisable ones included; the table is run at two base offsets).

NoisyLinear: the training-mode output equals torch.addmm over the reference's effective
parameters bit for bit; gx and the four parameter gradients against f64 autograd of the
reference formulation on the same f32 inputs under tests/test_gpu_mlp_bwd.py's rule: the error
over max|ref| may be 4 x that of torch's f32 autograd of the same formulation on the same
inputs, or the largest such torch error over the case list (the split-K gW is not bitwise
torch's).

Dueling: b in {1, 63, 64, 65, 257} x A in {1, 2, 6, 18} x N in {1, 2, 51, 64, 65, 200}, with
and without the softmax, against an f64 restatement on the same f32 inputs at
tests/test_gpu_dist_dqn.py's bounds: output rtol 1e-5, gradients rtol 1e-4, atol 1e-6 max|ref|
for both.  The torch fp32 formulation's own deviation is printed beside the kernel's.

Measured on an MI355X, as a fraction of max|ref|.  Dueling, the maxima over all 240 cases:
kernel out 5.44e-8, g_q 2.04e-7, g_v 8.82e-6 (torch fp32: 3.07e-7, 6.56e-7, 4.24e-6); the g_q
and g_v maxima are both at b 1, A 18, N 2 with the softmax, where g_v is a sum of 18 terms that
nearly cancel (kernel and torch alike start from the f32-rounded softmax output); at every
other case the kernel's g_v stays below 1.1e-7 and its g_q below 1.3e-7.  NoisyLinear: gx and
the four parameter gradients deviate from f64 exactly as torch's f32 autograd does at these
shapes (the largest, gx at (257, 130): 3.83e-7 for both).  tsrl_noisy_eps / _weights / _grads:
bit-equal at every size, shape and alignment."""
import pytest
import torch

from tianshou_amd import _C
from tianshou_amd.utils.net import NoisyLinear, _DuelingFn, dueling_combine

pytestmark = pytest.mark.gpu

for _name in ("tsrl_noisy_eps", "tsrl_noisy_weights", "tsrl_noisy_grads", "tsrl_dueling_fwd",
              "tsrl_dueling_bwd"):
    assert _name in _C.EXPORTED

CANARY = -12345.0
NCAN = 16
EPS_SIZES = (1, 3, 63, 64, 65, 257, 4099)
SHAPES = ((1, 1), (3, 5), (4, 64), (63, 65), (64, 64), (65, 3), (257, 130))  # (in, out)
BS = (1, 63, 64, 65, 257)
AS = (1, 2, 6, 18)
NS = (1, 2, 51, 64, 65, 200)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Arena:
    """Consecutive f32 views of one flat device buffer, NCAN canary words between them."""

    def __init__(self, words, dev, shift=0):
        self.flat = torch.full((words + shift,), CANARY, dtype=torch.float32, device=dev)
        self.o = shift
        self.guards = []

    def take(self, shape, fill=None, guard=False):
        n = 1
        for s in shape:
            n *= s
        if guard:
            self.o += NCAN
        v = self.flat[self.o:self.o + n].view(shape)
        if fill is not None:
            v.copy_(fill)
        if guard:
            self.guards.append((self.o, n))
        self.o += n + (NCAN if guard else 0)
        return v

    def guards_ok(self):
        return all(bool((self.flat[o - NCAN:o] == CANARY).all()) and
                   bool((self.flat[o + n:o + n + NCAN] == CANARY).all()) for o, n in self.guards)


def _layer_words(fin, fout):
    return 2 * fin * fout + 2 * fout + fin + fout + fin * fout + fout + 4 * NCAN


def _make_layer(arena, fin, fout, g):
    """(inputs dict, outputs dict) of one layer inside ``arena``."""
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(mu_w=arena.take((fout, fin), r(fout, fin)),
             sigma_w=arena.take((fout, fin), 0.1 * r(fout, fin)),
             mu_b=arena.take((fout,), r(fout)), sigma_b=arena.take((fout,), 0.1 * r(fout)),
             eps_p=arena.take((fin,), r(fin)), eps_q=arena.take((fout,), r(fout)))
    t["w_eff"] = arena.take((fout, fin), guard=True)
    t["b_eff"] = arena.take((fout,), guard=True)
    return t


def _table(layers, dev):
    rows = [[t[k].data_ptr() for k in ("mu_w", "sigma_w", "mu_b", "sigma_b", "eps_p", "eps_q",
                                      "w_eff", "b_eff")] + list(t["mu_w"].shape[::-1])
            for t in layers]
    assert len(rows[0]) == _C.NOISY_DESC_WORDS
    return torch.tensor(rows, dtype=torch.int64).to(dev)


def _run_weights(layers, dev):
    table = _table(layers, dev)
    _C.check(_C.lib().tsrl_noisy_weights(_C.ptr(table), len(layers),
                                         max(t["mu_w"].numel() for t in layers),
                                         _C.stream_ptr(dev)), "tsrl_noisy_weights")
    torch.cuda.synchronize()


def _check_weights(t):
    w_ref = t["mu_w"] + t["sigma_w"] * t["eps_q"].ger(t["eps_p"])
    b_ref = t["mu_b"] + t["sigma_b"] * t["eps_q"].clone()
    assert torch.equal(_bits(t["w_eff"]), _bits(w_ref)), tuple(t["mu_w"].shape)
    assert torch.equal(_bits(t["b_eff"]), _bits(b_ref)), tuple(t["mu_w"].shape)


# -- tsrl_noisy_eps --------------------------------------------------------------------------------
def _eps(x):
    n = x.numel()
    buf = torch.full((n + 2 * NCAN,), CANARY, dtype=torch.float32, device=x.device)
    _C.check(_C.lib().tsrl_noisy_eps(_C.ptr(x), n, buf[NCAN:].data_ptr(),
                                     _C.stream_ptr(x.device)), "tsrl_noisy_eps")
    assert bool((buf[:NCAN] == CANARY).all()) and bool((buf[NCAN + n:] == CANARY).all())
    return buf[NCAN:NCAN + n]


@pytest.mark.parametrize("n", EPS_SIZES)
def test_noisy_eps_is_torch_bit_for_bit(dev, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.1754944e-38, 3.0])
    for i in range(min(n, len(special))):  # +-0, +-subnormal, the smallest normal
        x[(i * 37) % n] = special[i]
    if n == 1:
        x[0] = -0.0
    x = x.to(dev)
    assert n < 3 or (bool((x == 0).any()) and bool(((x.abs() > 0) & (x.abs() < 1e-38)).any()))
    want = x.sign().mul_(x.abs().sqrt_())
    assert torch.equal(_bits(_eps(x)), _bits(want))


def test_noisy_eps_special_values_and_empty(dev):
    x = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e-45, float("inf"), float("-inf"), 4.0, -9.0,
                      float("nan")], device=dev)
    got = _eps(x)
    want = x.sign().mul_(x.abs().sqrt_())
    assert torch.equal(_bits(got[:-1]), _bits(want[:-1])) and bool(got[-1].isnan())
    assert got[7].item() == 2.0 and got[8].item() == -3.0
    assert _bits(got[:2]).tolist() == [0, 0]  # sign(+-0) is +0: no negative zero comes out
    assert _C.lib().tsrl_noisy_eps(None, 0, None, _C.stream_ptr(dev)) == 0


# -- tsrl_noisy_weights ----------------------------------------------------------------------------
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_noisy_weights_one_layer(dev, fin, fout):
    g = torch.Generator().manual_seed(1000 * fin + fout)
    arena = Arena(_layer_words(fin, fout), dev)
    t = _make_layer(arena, fin, fout, g)
    _run_weights([t], dev)
    _check_weights(t)
    assert arena.guards_ok()


@pytest.mark.parametrize("shift", (0, 1))
def test_noisy_weights_one_table_over_a_flat_buffer(dev, shift):
    g = torch.Generator().manual_seed(77 + shift)
    arena = Arena(sum(_layer_words(*s) for s in SHAPES), dev, shift)
    layers = [_make_layer(arena, fin, fout, g) for fin, fout in SHAPES]
    align = [(t["mu_w"].data_ptr() % 16, t["w_eff"].data_ptr() % 16) for t in layers]
    print("byte offsets mod 16 of (mu_w, w_eff) per layer:", align)
    # the vectorisable shapes meet both an aligned and a 4-byte-only start over the two shifts
    assert any(a != (0, 0) for a in align)
    _run_weights(layers, dev)
    for t in layers:
        _check_weights(t)
    assert arena.guards_ok()
    assert _C.lib().tsrl_noisy_weights(None, 0, 0, _C.stream_ptr(dev)) == 0


def test_noisy_weights_vector_path_is_taken_and_refused(dev):
    """(64, 64) at a 16-byte base takes the float4 path, one word further the scalar one; both
    give the same bits."""
    outs = []
    for shift in (0, 1):
        g = torch.Generator().manual_seed(5)
        arena = Arena(_layer_words(64, 64) + 8, dev, shift)
        t = _make_layer(arena, 64, 64, g)
        outs.append(t)
        _run_weights([t], dev)
        _check_weights(t)
        assert arena.guards_ok()
    assert outs[0]["mu_w"].data_ptr() % 16 == 0 and outs[0]["w_eff"].data_ptr() % 16 == 0
    assert outs[1]["mu_w"].data_ptr() % 16 == 4
    assert torch.equal(outs[0]["w_eff"], outs[1]["w_eff"])


# -- tsrl_noisy_grads ------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("fin,fout", SHAPES)
def test_noisy_grads_are_autograd_bit_for_bit(dev, fin, fout, shift):
    g = torch.Generator().manual_seed(2000 * fin + fout)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    arena = Arena(3 * fin * fout + 4 * fout + fin + 4 * NCAN, dev, shift)
    gw, gb = arena.take((fout, fin), r(fout, fin)), arena.take((fout,), r(fout))
    eps_p, eps_q = arena.take((fin,), r(fin)), arena.take((fout,), r(fout))
    gsw, gsb = arena.take((fout, fin), guard=True), arena.take((fout,), guard=True)
    _C.check(_C.lib().tsrl_noisy_grads(gw.data_ptr(), gb.data_ptr(), eps_p.data_ptr(),
                                       eps_q.data_ptr(), fin, fout, gsw.data_ptr(),
                                       gsb.data_ptr(), _C.stream_ptr(dev)), "tsrl_noisy_grads")
    mu_w, sigma_w, mu_b, sigma_b = (x.to(dev).requires_grad_(True) for x in
                                    (r(fout, fin), r(fout, fin), r(fout), r(fout)))
    weight = mu_w + sigma_w * eps_q.ger(eps_p)
    bias = mu_b + sigma_b * eps_q.clone()
    g_mu_w, g_sigma_w, g_mu_b, g_sigma_b = torch.autograd.grad(
        (weight, bias), (mu_w, sigma_w, mu_b, sigma_b), (gw, gb))
    assert torch.equal(g_mu_w, gw) and torch.equal(g_mu_b, gb)  # mu's gradients are gW, gb
    assert torch.equal(_bits(gsw), _bits(g_sigma_w)) and torch.equal(_bits(gsb), _bits(g_sigma_b))
    assert arena.guards_ok()


# -- NoisyLinear -----------------------------------------------------------------------------------
def _layer(fin, fout, dev, seed):
    torch.manual_seed(seed)
    layer = NoisyLinear(fin, fout, 0.5).to(dev)
    with torch.no_grad():  # sigma away from its constant initial value
        layer.sigma_W.mul_(1 + 0.5 * torch.randn_like(layer.sigma_W))
        layer.sigma_bias.mul_(1 + 0.5 * torch.randn_like(layer.sigma_bias))
    return layer


def _reference_layer(layer, x, gy, dtype):
    """(y, gx, g_mu_W, g_sigma_W, g_mu_bias, g_sigma_bias) of discrete.py:369-379 in dtype."""
    p = [t.detach().to(dtype).requires_grad_(True) for t in
         (layer.mu_W, layer.sigma_W, layer.mu_bias, layer.sigma_bias)]
    eps_p, eps_q = layer.eps_p.to(dtype), layer.eps_q.to(dtype)
    x = x.detach().to(dtype).requires_grad_(True)
    weight = p[0] + p[1] * eps_q.ger(eps_p)
    bias = p[2] + p[3] * eps_q.clone()
    y = torch.nn.functional.linear(x, weight, bias)
    return (y.detach(),) + torch.autograd.grad(y, [x] + p, gy.to(dtype))


def _layer_case(fin, fout, dev):
    b = 37
    layer = _layer(fin, fout, dev, 3000 * fin + fout)
    g = torch.Generator().manual_seed(fin + fout)
    x = torch.randn(b, fin, generator=g).to(dev).requires_grad_(True)
    gy = torch.randn(b, fout, generator=g).to(dev)
    return layer, x, gy


def _scaled_err(got, ref64):
    return float((got.double() - ref64).abs().max()) / (float(ref64.abs().max()) or 1.0)


@pytest.fixture(scope="module")
def torch_floor(dev):
    """The largest error of torch's f32 autograd of the reference formulation against f64 over
    the case list, per output."""
    worst = [0.0] * 5
    for fin, fout in SHAPES:
        layer, x, gy = _layer_case(fin, fout, dev)
        ref = _reference_layer(layer, x, gy, torch.float64)
        f32 = _reference_layer(layer, x, gy, torch.float32)
        worst = [max(w, _scaled_err(a, r)) for w, a, r in zip(worst, f32[1:], ref[1:])]
    return worst


@pytest.mark.parametrize("fin,fout", SHAPES)
def test_noisy_linear_forward_and_gradients(dev, torch_floor, fin, fout):
    layer, x, gy = _layer_case(fin, fout, dev)
    assert layer.training and layer.fused
    y = layer(x)
    w_ref = layer.mu_W + layer.sigma_W * layer.eps_q.ger(layer.eps_p)
    b_ref = layer.mu_bias + layer.sigma_bias * layer.eps_q.clone()
    assert torch.equal(y, torch.addmm(b_ref, x, w_ref.t()))
    assert torch.equal(layer._W_eff, w_ref) and torch.equal(layer._b_eff, b_ref)
    got = torch.autograd.grad(y, [x, layer.mu_W, layer.sigma_W, layer.mu_bias,
                                  layer.sigma_bias], gy)
    ref = _reference_layer(layer, x, gy, torch.float64)
    f32 = _reference_layer(layer, x, gy, torch.float32)
    names = ("gx", "g_mu_W", "g_sigma_W", "g_mu_bias", "g_sigma_bias")
    for name, a, t, r, floor in zip(names, got, f32[1:], ref[1:], torch_floor):
        err, terr = _scaled_err(a, r), _scaled_err(t, r)
        print(f"in {fin} out {fout} {name}: layer {err:.2e} torch-f32 {terr:.2e} of max|ref| "
              f"(floor {floor:.2e})")
        assert err <= max(4 * terr, floor), (name, err, terr, floor)
    # the sigma gradients are the mu gradients times the noise, rounded as autograd rounds
    assert torch.equal(got[2], got[1] * layer.eps_q.ger(layer.eps_p))
    assert torch.equal(got[4], got[3] * layer.eps_q)
    # eval mode: mu alone; fused = False: the reference's formulation
    layer.eval()
    assert torch.equal(layer(x), torch.nn.functional.linear(x, layer.mu_W, layer.mu_bias))
    layer.train()
    layer.fused = False
    assert torch.equal(layer(x), torch.nn.functional.linear(x, w_ref, b_ref))
    assert set(layer.state_dict()) == {"mu_W", "sigma_W", "mu_bias", "sigma_bias", "eps_p",
                                       "eps_q"}


# -- dueling ---------------------------------------------------------------------------------------
def dueling_reference(q, v, g, softmax):
    """common.py:276-284 in the dtype of q: (out, g_q, g_v) for the output gradient g."""
    q = q.detach().clone().requires_grad_(True)
    v = v.detach().clone().requires_grad_(True)
    out = q - q.mean(dim=1, keepdim=True) + v
    if softmax:
        out = torch.softmax(out, dim=-1)
    g_q, g_v = torch.autograd.grad(out, (q, v), g)
    return out.detach(), g_q, g_v


def dueling_inputs(b, A, N, dev):
    gen = torch.Generator().manual_seed(10000 * b + 100 * A + N)
    q = 2.0 * torch.randn(b, A, N, generator=gen)
    v = 2.0 * torch.randn(b, 1, N, generator=gen)
    g = torch.randn(b, A, N, generator=gen)
    return q.to(dev), v.to(dev), g.to(dev)


def _dueling_kernel(q, v, g, softmax):
    q = q.clone().requires_grad_(True)
    v = v.clone().requires_grad_(True)
    out = _DuelingFn.apply(q, v, softmax)
    g_q, g_v = torch.autograd.grad(out, (q, v), g)
    return out.detach(), g_q, g_v


WORST = {}


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("b", BS)
def test_dueling_matches_f64(dev, b, A, N):
    q, v, g = dueling_inputs(b, A, N, dev)
    for softmax in (False, True):
        ref = dueling_reference(q.double(), v.double(), g.double(), softmax)
        f32 = dueling_reference(q, v, g, softmax)
        got = _dueling_kernel(q, v, g, softmax)
        devs = []
        for name, k, t, r, rtol in zip(("out", "g_q", "g_v"), got, f32, ref, (1e-5, 1e-4, 1e-4)):
            scale = float(r.abs().max()) or 1.0
            kd = float((k.double() - r).abs().max()) / scale
            td = float((t.double() - r).abs().max()) / scale
            devs.append(f"{name} {kd:.2e} / {td:.2e}")
            WORST[name] = max(WORST.get(name, 0.0), kd)
            WORST["torch " + name] = max(WORST.get("torch " + name, 0.0), td)
            torch.testing.assert_close(k.double(), r, rtol=rtol, atol=1e-6 * scale,
                                       msg=lambda m: f"b {b} A {A} N {N} {name}: {m}")
        print(f"b {b} A {A} N {N} softmax {int(softmax)}: kernel / torch-f32 deviation from "
              "f64, over max|ref|: " + ", ".join(devs))
        assert got[0].shape == (b, A, N) and got[2].shape == (b, 1, N)
        if softmax:
            torch.testing.assert_close(got[0].sum(-1), torch.ones(b, A, device=dev), rtol=0,
                                       atol=1e-5)
        for a, c in zip(got, _dueling_kernel(q, v, g, softmax)):  # a fixed summation order
            assert torch.equal(a, c)
    print("measured maxima so far:", {k: f"{x:.2e}" for k, x in WORST.items()})


def test_dueling_constructed_rows(dev):
    b, A, N = 5, 6, 51
    gen = torch.Generator().manual_seed(4)
    v = torch.randn(b, 1, N, generator=gen).to(dev)
    g = torch.randn(b, A, N, generator=gen).to(dev)
    # all-equal q over the actions: out = softmax(v) (and v itself without the softmax)
    q = torch.randn(b, 1, N, generator=gen).to(dev).expand(b, A, N).contiguous()
    out, _, _ = _dueling_kernel(q, v, g, True)
    torch.testing.assert_close(out, torch.softmax(v, -1).expand(b, A, N), rtol=1e-6, atol=0)
    out, g_q, g_v = _dueling_kernel(q, v, g, False)
    torch.testing.assert_close(out, v.expand(b, A, N), rtol=0, atol=1e-6)
    torch.testing.assert_close(g_v, g.sum(1, keepdim=True), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(g_q.sum(1), torch.zeros(b, N, device=dev), rtol=0, atol=1e-5)
    # A = 1: q cancels; out comes from v alone and g_q is exactly 0
    q1 = torch.randn(b, 1, N, generator=gen).to(dev)
    for softmax in (False, True):
        out, g_q, g_v = _dueling_kernel(q1, v, g[:, :1].contiguous(), softmax)
        want = torch.softmax(v, -1) if softmax else v
        torch.testing.assert_close(out, want, rtol=1e-6, atol=0)
        assert bool((g_q == 0).all())
        ref = dueling_reference(q1.double(), v.double(), g[:, :1].double(), softmax)
        torch.testing.assert_close(g_v.double(), ref[2], rtol=1e-4,
                                   atol=1e-6 * float(ref[2].abs().max()))
    # dueling_combine takes the kernels on the GPU and the torch lines when told to
    q, v2, _ = dueling_inputs(7, 3, 51, dev)
    for softmax in (False, True):
        fused = dueling_combine(q, v2, softmax)
        plain = dueling_combine(q, v2, softmax, fused=False)
        assert torch.equal(plain, dueling_reference(q, v2, torch.ones_like(q), softmax)[0])
        torch.testing.assert_close(fused, plain, rtol=1e-5, atol=1e-6)


def test_dueling_row_limit(dev):
    """A * N above TSRL_DUELING_MAX_ROW: the documented code, nothing launched (the outputs
    keep their fill), and dueling_combine takes the torch formulation."""
    A, N = 33, 125
    assert A * N == _C.DUELING_MAX_ROW + 29
    q, v, g = dueling_inputs(2, A, N, dev)
    out = torch.full_like(q, CANARY)
    L = _C.lib()
    rc = L.tsrl_dueling_fwd(_C.ptr(q), _C.ptr(v), 2, A, N, 1, _C.ptr(out), _C.stream_ptr(dev))
    assert rc == _C.ERR_DUELING_ROW and b"exceeds" in L.tsrl_last_error()
    g_q, g_v = torch.full_like(q, CANARY), torch.full_like(v, CANARY)
    rc = L.tsrl_dueling_bwd(_C.ptr(g), _C.ptr(q), 2, A, N, 1, _C.ptr(g_q), _C.ptr(g_v),
                            _C.stream_ptr(dev))
    assert rc == _C.ERR_DUELING_ROW
    torch.cuda.synchronize()
    assert bool((out == CANARY).all()) and bool((g_q == CANARY).all()) and \
        bool((g_v == CANARY).all())
    for softmax in (False, True):
        got = dueling_combine(q, v, softmax)
        assert torch.equal(got, dueling_reference(q, v, g, softmax)[0])
    # at the limit the kernels run
    q, v, g = dueling_inputs(2, 32, 128, dev)
    assert 32 * 128 == _C.DUELING_MAX_ROW
    ref = dueling_reference(q.double(), v.double(), g.double(), True)
    got = _dueling_kernel(q, v, g, True)
    for k, r, rtol in zip(got, ref, (1e-5, 1e-4, 1e-4)):
        torch.testing.assert_close(k.double(), r, rtol=rtol, atol=1e-6 * float(r.abs().max()))
    # b = 0 launches nothing
    assert L.tsrl_dueling_fwd(None, None, 0, A, 2, 1, None, _C.stream_ptr(dev)) == 0
