"""tsrl_replay_sample / tsrl_nstep_apply (csrc/replay.hip) and the fused sample of
VectorReplayBuffer.sample_nstep / BasePolicy.update.

* chain and returns against the reference's own outputs (tests/golden/replay.npz): the terminal
  rows equal ref.VecBufferIndex.next applied n - 1 times (the oracle is pinned to the reference
  in tests/test_replay.py), the returns equal the recorded ones bit for bit;
* payload rows bitwise against plain torch indexing of the storage, over the row widths at
  which copy_row changes path, pitched storage, partial last workgroups and duplicate / negative
  indices;
* the ring's edges, each by name, against the unfused path (tsrl_ring_step_index +
  tsrl_nstep_return, themselves pinned to the reference) and the property the edge is about;
* argument checks;
* through the classes: sample_nstep == sample, update() with fused_sample on == off, the
  counter, and no Tensor.cpu() between the sample and learn()."""
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests.conftest import GOLDEN
from tianshou_amd import _C

pytestmark = pytest.mark.gpu

for _name in ("tsrl_replay_sample", "tsrl_nstep_apply"):
    assert _name in _C.EXPORTED

DEV = "cuda"


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "replay.npz"))


def _apply(tq, coef, ret):
    tq = tq.reshape(tq.shape[0], -1).contiguous()
    out = torch.empty_like(tq)
    _C.check(_C.lib().tsrl_nstep_apply(_C.ptr(tq), _C.ptr(coef), _C.ptr(ret), tq.shape[0],
                                       tq.shape[1], int(tq.dtype == torch.float64), _C.ptr(out),
                                       _C.stream_ptr()), "tsrl_nstep_apply")
    return out


# -- chain and returns against the reference -----------------------------------------------------
def test_vector_buffer_chain_and_returns_match_reference(z):
    from tianshou_amd.data import Batch, VectorReplayBuffer
    E, S = 6, 40
    vb = VectorReplayBuffer(E * S, E, device=DEV)
    ob = ref.VecBufferIndex(E * S, E)
    o = 0
    for k in z["nsv_add_len"]:
        sl = slice(o, o + k)
        ids, rew, te, tr = (z["nsv_add_" + s][sl] for s in ("ids", "rew", "term", "trunc"))
        vb.add(Batch(obs=np.zeros((k, 2), np.float32), act=np.zeros(k, np.int64), rew=rew,
                     terminated=te, truncated=tr, obs_next=np.zeros((k, 2), np.float32)),
               buffer_ids=ids)
        ob.add(rew, te, tr, ids)
        o += k
    idx = z["nsv_indices"]
    for n in (1, 3, 5, 12):
        vb._gather_nstep(idx, n, 0.97)
        p = vb._nstep_parts
        chain_end = idx % vb.maxsize
        for _ in range(n - 1):
            chain_end = ob.next(chain_end)
        terminal = p.token.terminal.cpu().numpy()
        np.testing.assert_array_equal(terminal, chain_end, err_msg=f"n={n}")
        np.testing.assert_array_equal(np.asarray(p.token), chain_end)
        for tag, tab in (("x1", z["nsv_table"][:, 0]), ("x3", z["nsv_table"]),
                         ("f64", z["nsv_table64"])):
            tq = torch.as_tensor(tab[terminal], device=DEV)
            want = z[f"nsv_n{n}_{tag}"]
            got = _apply(tq, p.coef, p.ret).cpu().numpy()
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=f"n={n} {tag}")


@pytest.mark.parametrize("tl", [0, 1])
def test_single_buffers_match_reference(z, tl):
    from tianshou_amd.data import Batch, ReplayBuffer
    buf = ReplayBuffer(10, device=DEV)
    for i in range(12):
        if tl:
            buf.add(Batch(obs=0, act=0, rew=i + 1, terminated=i % 4 == 3 and i != 3,
                          truncated=i == 3, info={"TimeLimit.truncated": i == 3}))
        else:
            buf.add(Batch(obs=0, act=0, rew=i + 1, terminated=i % 4 == 3, truncated=False))
    indices = buf.sample_indices(0)
    np.testing.assert_array_equal(indices, z[f"ns_tl{tl}_indices"])
    for n in (1, 2, 10):
        buf._gather_nstep(indices, n, 0.1)
        p = buf._nstep_parts
        nxt = buf.next(np.asarray(p.token))  # test/base/test_returns.py:137-140
        tq = -buf.rew[torch.as_tensor(nxt, device=DEV)].to(torch.float32)
        want = z[f"ns_tl{tl}_n{n}"]
        got = _apply(tq, p.coef, p.ret).cpu().numpy()
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=f"n={n}")


# -- payload, bitwise against torch indexing of the storage --------------------------------------
SIZE, NUM = 16, 2
M = SIZE * NUM


def _rand_bytes(rng, shape, dtype):
    t = torch.empty(shape, dtype=dtype)
    raw = rng.integers(0, 256, t.numel() * t.element_size(), dtype=np.uint8)
    return torch.as_tensor(raw).view(dtype).reshape(shape).to(DEV)


def _ring(rng):
    """Two sub-buffers of 16 rows: one full and wrapped (last write at row 5), one holding 9."""
    return dict(done=torch.as_tensor(rng.random(M) < 0.2, device=DEV),
                last=torch.as_tensor(np.array([5, SIZE + 8]), device=DEV),
                lengths=torch.as_tensor(np.array([SIZE, 9]), device=DEV))


def _np_next(i, done, last, lengths):
    b = i // SIZE
    start, cur = b * SIZE, np.maximum(1, lengths[b])
    end = done[i] | (i == last[b])
    return (i - start + 1 - end) % cur + start


def _launch(obs, obs_next, act, ring, idx, n_step, gamma=0.9, want_next=True, bad=None):
    """tsrl_replay_sample on raw storage tensors; returns the outputs by name."""
    bsz = int(idx.numel())
    dev = obs.device
    rng = np.random.default_rng(99)
    rew = torch.as_tensor(rng.standard_normal(M), device=dev)
    term = torch.as_tensor(rng.random(M) < 0.3, device=dev) & ring["done"]
    trunc = ring["done"] & ~term
    env_id = torch.arange(M, device=dev) // SIZE
    out = dict(
        obs=torch.empty((bsz,) + tuple(obs.shape[1:]), dtype=obs.dtype, device=dev),
        act=torch.empty((bsz,) + tuple(act.shape[1:]), dtype=act.dtype, device=dev),
        rew=torch.empty(bsz, dtype=torch.float64, device=dev),
        terminated=torch.empty(bsz, dtype=torch.bool, device=dev),
        truncated=torch.empty(bsz, dtype=torch.bool, device=dev),
        done=torch.empty(bsz, dtype=torch.bool, device=dev),
        env_id=torch.empty(bsz, dtype=torch.int64, device=dev),
        terminal=torch.empty(bsz, dtype=torch.int64, device=dev),
        ret=torch.empty(bsz, dtype=torch.float64, device=dev),
        coef=torch.empty(bsz, dtype=torch.float64, device=dev))
    out["obs_next"] = torch.empty_like(out["obs"]) if want_next else None
    out["term_obs_next"] = out["obs_next"] if n_step == 1 and want_next \
        else torch.empty_like(out["obs"])
    a = _C.ReplaySampleArgs()
    a.idx, a.bsz = _C.ptr(idx), bsz
    a.done, a.last_index, a.lengths = _C.ptr(ring["done"]), _C.ptr(ring["last"]), \
        _C.ptr(ring["lengths"])
    a.size, a.num, a.n_step, a.gamma = SIZE, NUM, n_step, gamma
    esz = obs.element_size()
    a.obs, a.obs_next = _C.ptr_rows(obs), _C.ptr_rows(obs_next)
    a.obs_row_bytes = esz * int(np.prod(obs.shape[1:]))
    a.obs_pitch = obs.stride(0) * esz if obs.dim() >= 2 else esz
    a.act, a.act_row_bytes = _C.ptr(act), act.element_size() * int(np.prod(act.shape[1:]))
    a.rew, a.terminated, a.truncated, a.env_id = _C.ptr(rew), _C.ptr(term), _C.ptr(trunc), \
        _C.ptr(env_id)
    a.obs_out, a.act_out, a.rew_out = _C.ptr(out["obs"]), _C.ptr(out["act"]), _C.ptr(out["rew"])
    a.terminated_out, a.truncated_out, a.done_out = _C.ptr(out["terminated"]), \
        _C.ptr(out["truncated"]), _C.ptr(out["done"])
    a.env_id_out, a.obs_next_out = _C.ptr(out["env_id"]), _C.ptr(out["obs_next"])
    a.terminal_out, a.term_obs_next_out = _C.ptr(out["terminal"]), _C.ptr(out["term_obs_next"])
    a.ret_out, a.coef_out = _C.ptr(out["ret"]), _C.ptr(out["coef"])
    for k, v in (bad or {}).items():
        setattr(a, k, v)
    _C.check(_C.lib().tsrl_replay_sample(a, _C.stream_ptr(dev)), "tsrl_replay_sample")
    out["_storage"] = dict(rew=rew, terminated=term, truncated=trunc, env_id=env_id)
    return out


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _padded(rng, d):
    """The buffer's wide-row storage: [M, d] view of [M, ceil(d / 32) * 32] f32."""
    return _rand_bytes(rng, (M, (d + 31) // 32 * 32), torch.float32)[:, :d]


OBS = {
    "f32_d2": lambda rng: _rand_bytes(rng, (M, 2), torch.float32),          # 8-byte rows
    "f32_d17": lambda rng: _rand_bytes(rng, (M, 17), torch.float32),        # 68 bytes: 4-byte copy
    "f32_d8": lambda rng: _rand_bytes(rng, (M, 8), torch.float32),          # 32 bytes, aligned
    "f32_d376_pitched": lambda rng: _padded(rng, 376),                      # pitch 1536, row 1504
    "u8_7": lambda rng: _rand_bytes(rng, (M, 7), torch.uint8),              # byte copy
}
ACT = {
    "i64": lambda rng: _rand_bytes(rng, (M,), torch.int64),
    "f32_6": lambda rng: _rand_bytes(rng, (M, 6), torch.float32),
    "f32_17": lambda rng: _rand_bytes(rng, (M, 17), torch.float32),
}


def _check_payload(obs, obs_next, act, idx_np, n_step, seed):
    rng = np.random.default_rng(seed)
    ring = _ring(rng)
    idx = torch.as_tensor(idx_np, device=DEV)
    out = _launch(obs, obs_next, act, ring, idx, n_step)
    c0 = torch.as_tensor(idx_np % M, device=DEV)
    done, last, lengths = (ring[k].cpu().numpy() for k in ("done", "last", "lengths"))
    term = idx_np % M
    for _ in range(n_step - 1):
        term = _np_next(term, done, last, lengths)
    np.testing.assert_array_equal(out["terminal"].cpu().numpy(), term)
    assert _same_bytes(out["obs"], obs[c0])
    assert _same_bytes(out["act"], act[c0])
    assert _same_bytes(out["obs_next"], obs_next[c0])
    assert _same_bytes(out["term_obs_next"], obs_next[torch.as_tensor(term, device=DEV)])
    for k, st in out["_storage"].items():
        assert torch.equal(out[k], st[c0]), k
    assert torch.equal(out["done"], ring["done"][c0])
    return out


@pytest.mark.parametrize("bsz", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("obs_kind", list(OBS))
def test_payload_rows_match_torch_indexing(obs_kind, bsz):
    rng = np.random.default_rng(bsz)
    obs, obs_next = OBS[obs_kind](rng), OBS[obs_kind](rng)
    act = list(ACT.values())[bsz % 3](rng)
    idx = rng.integers(0, M, bsz)  # 257 draws from 32 rows: duplicates
    for n_step in (1, 3):
        _check_payload(obs, obs_next, act, idx, n_step, seed=bsz + n_step)


@pytest.mark.parametrize("act_kind", list(ACT))
def test_payload_action_shapes(act_kind):
    rng = np.random.default_rng(3)
    obs, obs_next = OBS["f32_d17"](rng), OBS["f32_d17"](rng)
    _check_payload(obs, obs_next, ACT[act_kind](rng), rng.integers(0, M, 37), 2, seed=4)


def test_payload_atari_frames():
    rng = np.random.default_rng(6)
    obs = _rand_bytes(rng, (M, 4, 84, 84), torch.uint8)
    obs_next = _rand_bytes(rng, (M, 4, 84, 84), torch.uint8)
    _check_payload(obs, obs_next, ACT["i64"](rng), np.array([3, 31, 3, 0, 17]), 3, seed=7)


def test_payload_duplicate_and_negative_indices():
    rng = np.random.default_rng(8)
    obs, obs_next = OBS["f32_d8"](rng), OBS["f32_d8"](rng)
    idx = np.array([5, 5, 5, -1, -M, -7, 5, M - 1])
    _check_payload(obs, obs_next, ACT["f32_6"](rng), idx, 4, seed=9)


def test_payload_optional_one_step_next():
    """obs_next_out NULL: skipped; the terminal rows' next observation is still written."""
    rng = np.random.default_rng(10)
    obs, obs_next = OBS["f32_d8"](rng), OBS["f32_d8"](rng)
    idx = torch.as_tensor(rng.integers(0, M, 9), device=DEV)
    for n_step in (1, 3):
        ring = _ring(np.random.default_rng(11))
        out = _launch(obs, obs_next, ACT["i64"](rng), ring, idx, n_step, want_next=False)
        assert out["obs_next"] is None
        assert _same_bytes(out["term_obs_next"], obs_next[out["terminal"]])


# -- ring edges, through the buffer, against the unfused path ----------------------------------
def _vec_buffer(E, S, steps, done_at=(), term_at=(), envs=None, D=3, **kw):
    """E sub-buffers of S rows; ``steps`` adds to ``envs`` (default all); (step, env) pairs in
    done_at end an episode, those also in term_at as terminated."""
    from tianshou_amd.data import Batch, VectorReplayBuffer
    buf = VectorReplayBuffer(E * S, E, device=DEV, **kw)
    ids = np.arange(E) if envs is None else np.asarray(envs)
    rng = np.random.default_rng(17)
    for t in range(steps):
        k = len(ids)
        done = np.array([(t, e) in done_at for e in ids])
        term = np.array([(t, e) in term_at for e in ids])
        buf.add(Batch(obs=rng.standard_normal((k, D)).astype(np.float32),
                      act=rng.integers(0, 4, k), rew=rng.standard_normal(k), terminated=term,
                      truncated=done & ~term,
                      obs_next=rng.standard_normal((k, D)).astype(np.float32)), buffer_ids=ids)
    return buf


def _fused_vs_unfused(buf, idx, n_step, gamma=0.9):
    """Fused sample + tsrl_nstep_apply against __getitem__ + the unfused compute_nstep_return;
    returns (parts, terminal rows) of the fused sample."""
    from tianshou_amd.data import Batch
    from tianshou_amd.policy import BasePolicy
    idx = np.asarray(idx, np.int64)
    table = torch.as_tensor(np.random.default_rng(1).standard_normal((buf.maxsize, 2)),
                            device=DEV).float()
    seen = []

    def fn(buffer, indices):
        seen.append(indices)
        return table[torch.as_tensor(np.asarray(indices), device=DEV)]
    plain = buf[idx]
    old = BasePolicy.compute_nstep_return(Batch(), buf, idx, fn, gamma=gamma, n_step=n_step)
    before = buf.fused_samples
    batch = buf._gather_nstep(idx, n_step, gamma)
    parts = buf._nstep_parts
    assert buf.fused_samples == before + 1 and parts.indices is idx
    new = BasePolicy.compute_nstep_return(batch, buf, idx, fn, gamma=gamma, n_step=n_step)
    assert buf._nstep_parts is None  # taken
    assert isinstance(seen[0], np.ndarray) and seen[1] is parts.token
    terminal = np.asarray(parts.token)
    np.testing.assert_array_equal(terminal, seen[0])
    walk = idx % buf.maxsize
    for _ in range(n_step - 1):
        walk = buf.next(walk)
    np.testing.assert_array_equal(terminal, walk)
    assert _same_bytes(new.returns, old.returns)
    for k in ("obs", "act", "rew", "terminated", "truncated", "done", "obs_next"):
        assert batch[k].dtype == plain[k].dtype and _same_bytes(batch[k], plain[k]), k
    assert torch.equal(batch.info.env_id, plain.info.env_id)
    want_next = buf[terminal].obs_next
    if buf._save_obs_next:  # else get() has no such key, with a token as with indices
        assert _same_bytes(buf.get(parts.token, "obs_next"), want_next)
    assert _same_bytes(buf[parts.token].obs_next, want_next)
    assert _same_bytes(buf[parts.token].act, buf[terminal].act)
    return parts, terminal


def test_edge_empty_sub_buffer():
    buf = _vec_buffer(3, 8, 5, envs=[0, 2])
    assert buf._lengths.tolist() == [5, 0, 5]
    _fused_vs_unfused(buf, [0, 4, 16, 20, 8, 11], 3)  # rows 8, 11: the empty sub-buffer


def test_edge_wrapped_sub_buffer():
    buf = _vec_buffer(2, 8, 13, done_at={(9, 0)})
    assert buf._index_per_env.tolist() == [5, 5] and buf._lengths.tolist() == [8, 8]
    _, terminal = _fused_vs_unfused(buf, np.arange(16), 4)
    assert terminal[6] == 1  # 6 -> 7 -> 0 -> 1: across the storage end


def test_edge_index_at_last_index():
    buf = _vec_buffer(2, 8, 6)
    last = buf.last_index.copy()
    parts, terminal = _fused_vs_unfused(buf, last, 5)
    np.testing.assert_array_equal(terminal, last)  # next(i) == i on the unfinished row
    assert torch.equal(parts.ret, buf.rew[torch.as_tensor(last, device=DEV)])
    assert parts.coef.tolist() == [0.9, 0.9]  # gammas = 1


def test_edge_done_inside_window():
    buf = _vec_buffer(1, 16, 10, done_at={(4, 0)})
    parts, terminal = _fused_vs_unfused(buf, [2, 3, 4, 5], 5)
    assert terminal.tolist() == [4, 4, 4, 9]
    g = np.float64(0.9)
    assert parts.coef.tolist() == [g * g * g, g * g, g, g * g * g * g * g]


def test_edge_terminated_terminal_row_has_zero_coef():
    buf = _vec_buffer(1, 16, 10, done_at={(4, 0)}, term_at={(4, 0)})
    parts, terminal = _fused_vs_unfused(buf, [2, 6], 3)
    assert terminal.tolist() == [4, 8]
    g = np.float64(0.9)
    assert parts.coef.tolist() == [0.0, g * g * g]
    assert not np.signbit(parts.coef.cpu().numpy()[0])


def test_edge_truncated_terminal_row_keeps_coef():
    buf = _vec_buffer(1, 16, 10, done_at={(4, 0)})
    assert bool(buf.truncated[4]) and not bool(buf.terminated[4])
    parts, terminal = _fused_vs_unfused(buf, [2], 3)
    g = np.float64(0.9)
    assert terminal.tolist() == [4] and parts.coef.tolist() == [g * g * g]


def test_edge_n_step_64_on_a_short_chain():
    buf = _vec_buffer(2, 80, 70, done_at={(9, 0)})
    parts, terminal = _fused_vs_unfused(buf, [3, 0, 80, 87], 64)
    assert terminal.tolist() == [9, 9, 80 + 63, 80 + 69]
    gp = np.float64(1.0)
    for _ in range(64):
        gp = gp * np.float64(0.9)
    assert parts.coef.tolist()[2] == gp  # a full 64-row chain


def test_edge_ignore_obs_next():
    buf = _vec_buffer(2, 8, 13, done_at={(9, 0)}, ignore_obs_next=True)
    assert "obs_next" not in buf._meta.keys()
    parts, terminal = _fused_vs_unfused(buf, np.arange(16), 3)
    nxt = buf.next(terminal)
    assert _same_bytes(parts.token.obs_next, buf.obs[torch.as_tensor(nxt, device=DEV)])


# -- argument checks -------------------------------------------------------------------------------
def test_argument_checks():
    rng = np.random.default_rng(2)
    obs, obs_next, act = OBS["f32_d8"](rng), OBS["f32_d8"](rng), ACT["i64"](rng)
    ring = _ring(rng)
    idx = torch.as_tensor(np.arange(5), device=DEV)
    for bad in (dict(n_step=0), dict(n_step=65), dict(idx=None), dict(obs_out=None),
                dict(coef_out=None), dict(terminal_out=None), dict(bsz=-1)):
        with pytest.raises(_C.TsrlError, match="tsrl_replay_sample"):
            _launch(obs, obs_next, act, ring, idx, 3, bad=bad)
    # bsz 0 launches nothing: not even the pointers are looked at
    out = _launch(obs, obs_next, act, ring, idx, 3, bad=dict(bsz=0, obs=None))
    torch.cuda.synchronize()
    L = _C.lib()
    tq = torch.zeros(4, device=DEV)
    co = torch.zeros(4, dtype=torch.float64, device=DEV)
    with pytest.raises(_C.TsrlError, match="tsrl_nstep_apply"):
        _C.check(L.tsrl_nstep_apply(_C.ptr(tq), None, _C.ptr(co), 4, 1, 0, _C.ptr(tq),
                                    _C.stream_ptr()), "tsrl_nstep_apply")
    with pytest.raises(_C.TsrlError, match="tsrl_nstep_apply"):
        _C.check(L.tsrl_nstep_apply(_C.ptr(tq), _C.ptr(co), _C.ptr(co), 4, 0, 0, _C.ptr(tq),
                                    _C.stream_ptr()), "tsrl_nstep_apply")
    assert L.tsrl_nstep_apply(None, None, None, 0, 1, 0, None, _C.stream_ptr()) == 0
    assert out["obs"].shape[0] == 5


# -- through the classes --------------------------------------------------------------------------
def _same_batches(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a.keys():
        if k in ("info", "policy"):
            assert list(a[k].keys()) == list(b[k].keys()), k
            for kk in a[k].keys():
                assert a[k][kk].dtype == b[k][kk].dtype and _same_bytes(a[k][kk], b[k][kk]), kk
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert _same_bytes(a[k], b[k]), k


@pytest.mark.parametrize("per", [False, True])
def test_sample_nstep_equals_sample(per):
    from tianshou_amd.data import Batch, PrioritizedVectorReplayBuffer, VectorReplayBuffer
    E, S = 4, 12
    buf = PrioritizedVectorReplayBuffer(E * S, E, alpha=0.6, beta=0.4, device=DEV) if per \
        else VectorReplayBuffer(E * S, E, device=DEV)
    rng = np.random.default_rng(21)
    for t in range(17):
        done = rng.random(E) < 0.2
        buf.add(Batch(obs=rng.standard_normal((E, 5)).astype(np.float32),
                      act=rng.standard_normal((E, 2)).astype(np.float32),
                      rew=rng.standard_normal(E), terminated=done & (rng.random(E) < 0.5),
                      truncated=np.zeros(E, bool),
                      obs_next=rng.standard_normal((E, 5)).astype(np.float32),
                      info=Batch(extra=rng.integers(0, 9, E)),
                      policy=Batch(h=rng.standard_normal((E, 3)).astype(np.float32))),
                buffer_ids=np.arange(E))
    if per:
        buf.update_weight(np.arange(20), torch.as_tensor(rng.random(20), device=DEV))
    for bs, n in ((7, 1), (33, 3)):
        np.random.seed(5)
        want, want_idx = buf.sample(bs)
        np.random.seed(5)
        before = buf.fused_samples
        got, got_idx = buf.sample_nstep(bs, n, 0.99)
        assert buf.fused_samples == before + 1
        np.testing.assert_array_equal(got_idx, want_idx)
        assert ("weight" in got.keys()) == per
        _same_batches(got, want)
    # what the kernel cannot serve is sample(): the whole buffer in order
    got, got_idx = buf.sample_nstep(0, 3, 0.99)
    np.testing.assert_array_equal(got_idx, buf.sample_indices(0))
    assert buf.fused_samples == before + 1


def _three_updates(make, fused):
    policy, buf, bs, seed, params = make()
    policy.fused_sample = fused
    from tests.test_gpu_ddpg import _record
    seen = _record(policy)
    np.random.seed(seed)
    torch.manual_seed(3)
    for _ in range(3):
        policy.update(bs, buf)
    return seen, params(policy), buf


def _make_dqn(golden_dir):
    from tests.test_gpu_dqn import _cfg, _filled_buffer, _policy
    z = np.load(os.path.join(golden_dir, "dqn.npz"))
    cfg = _cfg(z)

    def make():
        policy, v = _policy(z, cfg, "nature_huber", torch.device(DEV, 0))
        assert v["n_step"] == 3
        policy.train()
        buf = _filled_buffer(z, cfg, torch.device(DEV, 0))
        return policy, buf, v["bs"], cfg["seed"], lambda p: torch.cat(
            [t.detach().reshape(-1) for m in (p.model, p.model_old) for t in m.parameters()])
    return make


def _make_sac(golden_dir):
    from tests import sac_common
    from tests.test_gpu_ddpg import _filled_buffer
    z = sac_common.golden(golden_dir)
    cfg = sac_common.learn_cfg(z)

    def make():
        policy, v = sac_common.make_policy(z, cfg, "sac", torch.device(DEV, 0))
        assert v["n_step"] == 1
        policy.train()
        sac_common.feed_draws(policy, sac_common.update_draws(z, "sac"))
        buf = _filled_buffer(z, cfg, torch.device(DEV, 0))
        return policy, buf, v["bs"], cfg["seed"], lambda p: torch.as_tensor(
            sac_common.flat_params(p))
    return make


@pytest.mark.parametrize("kind", ["dqn_n3", "sac_n1"])
def test_update_fused_sample_on_equals_off(golden_dir, kind):
    make = (_make_dqn if kind == "dqn_n3" else _make_sac)(golden_dir)
    on, p_on, buf_on = _three_updates(make, True)
    off, p_off, buf_off = _three_updates(make, False)
    assert buf_on.fused_samples == 3 and buf_off.fused_samples == 0
    assert len(on) == len(off) == 3
    for a, b in zip(on, off):
        np.testing.assert_array_equal(a["indices"], b["indices"])
        assert a["returns"].dtype == b["returns"].dtype
        assert _same_bytes(a["returns"], b["returns"])
        td = "td_error" if "td_error" in a else "td"
        assert _same_bytes(a[td], b[td])
    assert _same_bytes(p_on, p_off)


def test_no_host_copy_between_sample_and_learn(golden_dir, monkeypatch):
    policy, buf, bs, seed, _ = _make_dqn(golden_dir)()
    calls, window = [], [False]
    real_cpu, real_sample, real_learn = torch.Tensor.cpu, buf.sample_nstep, policy.learn

    def spy(self, *a, **kw):
        if window[0]:
            calls.append(tuple(self.shape))
        return real_cpu(self, *a, **kw)

    def sample_nstep(*a, **kw):
        out = real_sample(*a, **kw)
        window[0] = True
        return out

    def learn(batch, **kw):
        window[0] = False
        return real_learn(batch, **kw)
    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    buf.sample_nstep, policy.learn = sample_nstep, learn
    np.random.seed(seed)
    for _ in range(3):
        policy.update(bs, buf)
    assert buf.fused_samples == 3 and calls == []
    # the unfused path reads the terminal rows back inside that window
    policy.fused_sample = False
    real = buf.sample

    def sample(*a, **kw):
        out = real(*a, **kw)
        window[0] = True
        return out
    buf.sample = sample
    policy.update(bs, buf)
    assert len(calls) >= 1 and buf.fused_samples == 3
