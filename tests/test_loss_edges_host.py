"""The references of tests/test_gpu_loss_edges.py against each other, on the CPU: for every
case the f64 reference and the torch-f32 formulation agree outside branch-ambiguous rows, at
most 1 % of a case's rows are ambiguous, the masked cases are finite, and the written-out
formulation is torch's own (torch.distributions, oracle/ref.py) at float32."""
import numpy as np
import pytest
import torch

from oracle import ref

from . import loss_edges_common as lc


def _close(got, want, name):
    fin = want[torch.isfinite(want)]
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4,
                               atol=1e-6 * float(fin.abs().max() if fin.numel() else 0.0)
                               + 1e-9, err_msg=name)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_references_agree(name):
    case = lc.CASES[name]
    r64, r32, amb = lc.refs(name)
    share = float(amb.double().mean())
    print(f"{name}: {int(amb.sum())} of {case['B']} rows branch-ambiguous")
    assert share <= 0.01
    if case.get("floor", True):  # (the ill-conditioned cases: f32 is far off by construction)
        keep = (~amb).numpy()
        for o in lc.outputs(case["kind"]):
            a, b = r32[o], r64[o].float()
            if o in lc.ROW_GRADS:
                a, b = a[keep], b[keep]
            _close(a, b, f"{name} {o}")
    if name.startswith("masked") or name in ("extreme", "one-action") or \
            name.startswith("probs"):
        for o in lc.outputs(case["kind"]):
            if o == "logp" and "masked_taken" in case:
                lp = r64[o].clone()
                assert lp[case["masked_taken"]] == -lc.INF
                lp[case["masked_taken"]] = 0.0
                assert torch.isfinite(lp).all()
                continue
            assert torch.isfinite(r64[o]).all() and torch.isfinite(r32[o]).all(), o


def test_masked_cases_cover_every_count():
    """Every number of masked entries 1 .. A-1 sits in a row whose taken action is unmasked;
    masked entries get gradient exactly 0 in the reference."""
    for name in lc.names("masked"):
        case = lc.CASES[name]
        assert set(case["masked_counts"]) == set(range(1, case["A"]))
        x, act = case["x"], case["act"]
        rows = torch.arange(case["B"])
        taken_masked = x[rows, act] == -lc.INF
        assert int(taken_masked.sum()) == (1 if "masked_taken" in case else 0)
        r64 = lc.refs(name)[0]
        assert bool((r64["grad_x"][x == -lc.INF] == 0).all())


@pytest.mark.parametrize("name", ["masked-ppo-B65-A6-ent0.01", "probs-ent0.01",
                                  "width-cat-B257-A33", "width-gauss-B257-A33",
                                  "gauss-edge", "extreme"])
def test_formulation_is_torchs(name):
    """loss_ref at float32 is oracle/ref.py's torch formulation (torch.distributions): the
    same terms bit for bit, the same gradients to a few roundings."""
    case = lc.CASES[name]
    p = case["p"]
    kw = dict(eps_clip=p["eps_clip"], dual_clip=p["dual_clip"] or None,
              value_clip=p["value_clip"], norm_adv=p["norm_adv"], vf_coef=p["vf_coef"],
              ent_coef=p["ent_coef"])
    mine = lc.refs(name)[1]
    if case["kind"] == "cat":
        want = ref.ppo_categorical_loss_torch(
            case["x"], case["value"], case["act"], case["logp_old"], case["adv"], case["ret"],
            case["v_s"], case["mode"], **kw)
        grads = dict(grad_x=want[4]["x"], grad_value=want[4]["value"])
    else:
        want = ref.ppo_gaussian_loss_torch(
            case["mu"], case["log_std"], case["value"], case["act"], case["logp_old"],
            case["adv"], case["ret"], case["v_s"], **kw)
        grads = dict(grad_mu=want[4]["mu"], grad_ls=want[4]["sigma_param"],
                     grad_value=want[4]["value"])
    for o, w in zip(lc.TERMS, want[:4]):
        assert torch.equal(mine[o], w), o
    for o, w in grads.items():
        # autograd sums a row's contributions in the order of its own graph: a few f32 roundings
        err = float((mine[o] - w).abs().max()) / float(w.abs().max())
        print(f"{name} {o}: {err:.2e} of max|grad| from oracle/ref.py")
        assert err <= 8 * 2.0 ** -24, o


def test_probs_pairs_scale():
    """A row times 3 has a third of the gradient (the reference's own / S)."""
    r64 = lc.refs("probs-ent0.01")[0]
    g = r64["grad_x"]
    torch.testing.assert_close(3 * g[lc.PAIRS:2 * lc.PAIRS], g[:lc.PAIRS], rtol=1e-12,
                               atol=1e-18)
