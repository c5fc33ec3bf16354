"""Host test of tests/mlp_common.py's fragment-layout writer (no GPU): rows_to_frag is the
inverse of frag_to_rows, which tests/test_gpu_mlp*.py hold against the kernels' own output."""
import pytest
import torch

from tests.mlp_common import frag_floats, frag_to_rows, rows_to_frag


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 128, 129, 257])
def test_rows_to_frag_inverts_frag_to_rows(n):
    """frag_to_rows(rows_to_frag(R), n) has R's bits (denormals, -0.0 and Inf included); the
    buffer has tsrl_mlp_frag_floats(n) floats, whole 128-row blocks; every float of the pad
    rows holds fill (finite, and NaN), and no other float does."""
    g = torch.Generator().manual_seed(n)
    R = torch.rand(n, 128, generator=g) + 0.5          # never equal to the fill
    R[0, 0], R[n - 1, 127], R[n // 2, 64] = 1e-40, -0.0, float("inf")
    numel = frag_floats(n)
    assert numel == (n + 127) // 128 * 128 * 128
    padded = numel // 128
    F = rows_to_frag(R, -7.0)
    assert F.shape == (numel,) and F.dtype == torch.float32
    assert torch.equal(_bits(frag_to_rows(F, n)), _bits(R))
    assert int((F == -7.0).sum()) == (padded - n) * 128
    if padded > n:
        assert bool((frag_to_rows(F, padded)[n:] == -7.0).all())
    Fn = rows_to_frag(R, float("nan"))
    assert torch.equal(_bits(frag_to_rows(Fn, n)), _bits(R))
    assert int(torch.isnan(Fn).sum()) == (padded - n) * 128
    if padded > n:
        assert bool(torch.isnan(frag_to_rows(Fn, padded)[n:]).all())


def test_rows_to_frag_places_one_element_at_frag_off4():
    """One element checked against x6.h frag_off4 written out by hand: row 37, feature 77 =
    row tile 1, feature tile 2, lane (37 & 31) + 32 h, feature 13 = rho(r) + 4 h with h = 1,
    rho(r) = 9 -> r = 5 (q = 1, e = 1): offset tile * 1024 + (q * 64 + lane) * 4 + e."""
    R = torch.zeros(40, 128)
    R[37, 77] = 3.0
    F = rows_to_frag(R, 0.0)
    tile, lane, q, e = 1 * 4 + 2, 5 + 32, 1, 1
    assert int(F.nonzero()) == tile * 1024 + (q * 64 + lane) * 4 + e
