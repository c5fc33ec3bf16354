"""policy/flat_learn.py's target mirror on host tensors: ``mirror_target`` makes a target
network's parameters views into one flat buffer laid out as the online network's flat
parameters, ``target_mirrored`` says whether that still holds.  Neither depends on a device, so
an f32 buffer with FlatAdam's ``_slot`` views stands in for FlatAdam.flat_param here (bind_adam
itself needs the HIP library).  The conv case keeps a channels_last weight: a slot that is not
contiguous."""
from copy import deepcopy

import pytest
import torch

from tianshou_amd.policy.flat_adam import _slot
from tianshou_amd.policy.flat_learn import mirror_target, target_mirrored


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
