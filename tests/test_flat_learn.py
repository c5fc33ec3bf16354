"""policy/flat_learn.py's target mirror on host tensors: ``mirror_target`` makes a target
network's parameters views into one flat buffer laid out as the online network's flat
parameters, ``target_mirrored`` says whether that still holds.  Neither depends on a device, so
an f32 buffer with FlatAdam's ``_slot`` views stands in for FlatAdam.flat_param here (bind_adam
itself needs the HIP library).  The conv case keeps a channels_last weight: a slot that is not
contiguous.  ``KernelGradLoss`` is the backward the off-policy loss functions inherit: a
stand-in forward that "writes" flat f32 gradients the way their kernels do exercises it."""
from copy import deepcopy

import pytest
import torch

from tianshou_amd.policy.flat_adam import _slot
from tianshou_amd.policy.flat_learn import (KernelGradLoss, _unit_seed, mirror_target,
                                            target_mirrored)


def _mlp():
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))


def _conv():
    net = torch.nn.Sequential(torch.nn.Conv2d(2, 3, 2), torch.nn.Flatten(),
                              torch.nn.Linear(12, 2))
    return net.to(memory_format=torch.channels_last)


def _flatten(net):
    """The online parameters moved into one flat f32 buffer, as FlatAdam.bind_adam lays them
    out; returns (params, flat)."""
    params = list(net.parameters())
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32)
    o = 0
    for p in params:
        v = _slot(flat, o, p)
        v.copy_(p.detach())
        with torch.no_grad():
            p.data = v
        o += p.numel()
    return params, flat


@pytest.mark.parametrize("make", (_mlp, _conv))
def test_target_mirror_layout_and_predicate(make):
    torch.manual_seed(0)
    net = make()
    old = deepcopy(net)
    with torch.no_grad():
        for p in old.parameters():  # the target's own values, not the online ones
            p.add_(1.0)
    before = [(p.detach().clone(), p.shape, p.stride()) for p in old.parameters()]
    params, flat = _flatten(net)
    if make is _conv:
        assert not params[0].is_contiguous()

    flat_old = mirror_target(old, params, flat)

    assert flat_old.shape == flat.shape and flat_old.dtype == flat.dtype
    assert flat_old.data_ptr() != flat.data_ptr()
    for p_old, p, (value, shape, stride) in zip(old.parameters(), params, before):
        assert p_old.untyped_storage().data_ptr() == flat_old.untyped_storage().data_ptr()
        assert p_old.storage_offset() == p.storage_offset()
        assert p_old.shape == shape == p.shape
        assert p_old.stride() == stride == p.stride()
        assert torch.equal(p_old, value) and not torch.equal(p_old, p)
    # one copy between the flat buffers is the hard sync
    flat_old.copy_(flat)
    for p_old, p in zip(old.parameters(), params):
        assert torch.equal(p_old, p)

    assert target_mirrored(old, flat_old, flat, flat)
    assert not target_mirrored(old, None, None, flat)
    # the source buffer object replaced (what a re-bound FlatAdam hands out)
    assert not target_mirrored(old, flat_old, flat, flat.clone())
    assert not target_mirrored(old, flat_old, flat, None)
    # one target parameter re-pointed elsewhere
    p = list(old.parameters())[-1]
    with torch.no_grad():
        p.data = p.data.clone()
    assert not target_mirrored(old, flat_old, flat, flat)
    # mirrored again, it holds again
    again = mirror_target(old, params, flat)
    assert target_mirrored(old, again, flat, flat)
    assert not target_mirrored(old, flat_old, flat, flat)


class _StandInLoss(KernelGradLoss):
    @staticmethod
    def forward(ctx, args, x, y):
        grads = [torch.full((t.numel(),), float(k + 2), dtype=torch.float32)
                 for k, t in enumerate((x, y))]
        KernelGradLoss.keep(ctx, grads, (x, y))
        return torch.zeros((), dtype=torch.float32)


def test_kernel_grad_loss_backward():
    def grads_after(seed):
        x = torch.zeros(3, 2, dtype=torch.float64, requires_grad=True)
        y = torch.zeros(4, requires_grad=True)
        _StandInLoss.apply(("not a tensor",), x, y).backward(seed)
        return x.grad, y.grad

    # scaled by the seed, viewed and cast to each input's shape and dtype
    gx, gy = grads_after(torch.tensor(0.5))
    assert gx.dtype == torch.float64 and torch.equal(gx, torch.full((3, 2), 1.0).double())
    assert gy.dtype == torch.float32 and torch.equal(gy, torch.full((4,), 1.5))
    # the unit seed hands the kernel's gradients over as they are
    gx, gy = grads_after(_unit_seed(torch.device("cpu")))
    assert torch.equal(gx, torch.full((3, 2), 2.0).double())
    assert torch.equal(gy, torch.full((4,), 3.0))
