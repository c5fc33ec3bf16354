"""tests/golden/dqn.npz (tools/gen_goldens.py gen_dqn: the reference DQNPolicy on CPU torch)
pinned on the host: a torch-CPU restatement of dqn.py:85-96,167-188 replays every learn
variant from the recorded sample indices (and, for the prioritized variant, the recorded
importance weights), and a NumPy restatement of exploration_noise (dqn.py:190-203) replays
every noise case including the NumPy stream position after the call.  This shows that the
recorded quantities suffice to replay a run; tests/test_gpu_dqn.py compares the device
DQNPolicy with the same file.

Tolerances: n-step returns exact in f32 (the same CPU torch forwards feed the f64 n-step
oracle, oracle/ref.py nstep_return); losses and parameters rtol 1e-6 (autograd's own kernels
against the reference's: same library, possibly another summation split)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests.conftest import GOLDEN


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "dqn.npz"))


def replay_adds(z):
    """The recorded add() stream as (ids, {key: rows}) per call."""
    o = 0
    for k in z["add_len"]:
        sl = slice(o, o + int(k))
        yield z["add_ids"][sl], {key: z["add_" + key][sl] for key in
                                 ("obs", "act", "rew", "terminated", "truncated", "obs_next")}
        o += int(k)


def host_buffer(z, cfg):
    vb = ref.VecBufferIndex(cfg["E"] * cfg["S"], cfg["E"])
    store = dict(obs=np.zeros((vb.maxsize, cfg["D"]), np.float32),
                 obs_next=np.zeros((vb.maxsize, cfg["D"]), np.float32),
                 act=np.zeros(vb.maxsize, np.int64), terminated=np.zeros(vb.maxsize, bool))
    for ids, row in replay_adds(z):
        ptr, *_ = vb.add(row["rew"], row["terminated"], row["truncated"], ids)
        for k in store:
            store[k][ptr] = row[k]
    return vb, store


def make_net(z, cfg, prefix="init_"):
    sizes = [cfg["D"], *cfg["hidden"], cfg["A"]]
    layers = []
    for i in range(len(sizes) - 1):
        layers += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    net = torch.nn.Sequential(*layers[:-1])
    load(net, z, prefix)
    return net


def param_keys(z, prefix):
    return sorted(k for k in z.files if k.startswith(prefix))


def load(net, z, prefix):
    keys = param_keys(z, prefix)
    sd = net.state_dict()
    assert len(keys) == len(sd)
    # both name lists sort into layer order with weight after bias inside a layer
    net.load_state_dict({n: torch.as_tensor(z[k]) for n, k in zip(sorted(sd), keys)})


def test_learn_variants_replay_from_recorded_indices(z):
    cfg = json.loads(str(z["learn_cfg"]))
    vb, store = host_buffer(z, cfg)
    np.testing.assert_array_equal(vb.sizes, z["buf_lengths"])
    np.testing.assert_array_equal(vb.last_index, z["buf_last_index"])
    assert (vb.sizes == cfg["S"]).sum() == 1  # the wrapped sub-buffer
    for tag, v in cfg["variants"].items():
        net = make_net(z, cfg)
        old = make_net(z, cfg) if v["freq"] > 0 else net
        if v["optim"] == "rms":
            optim = torch.optim.RMSprop(net.parameters(), lr=7e-4, eps=1e-5, alpha=0.99)
        else:
            optim = torch.optim.Adam(net.parameters(), lr=1e-3)
        for u in range(6):
            q = f"{tag}_u{u}_"
            idx = z[q + "indices"]
            assert len(idx) == v["bs"]
            # process_fn: dqn.py:85-96 at the chain's last row, then the n-step return
            terminal = idx % vb.maxsize
            for _ in range(v["n_step"] - 1):
                terminal = vb.next(terminal)
            s_next = torch.as_tensor(store["obs_next"][terminal])
            with torch.no_grad():
                q_new, q_old = net(s_next), old(s_next)
                if v["is_double"]:
                    tq = q_old[np.arange(len(idx)), q_new.max(dim=1)[1]]
                else:
                    tq = q_old.max(dim=1)[0]
            returns, _ = ref.nstep_return(vb, store["terminated"], idx, tq.numpy(),
                                          cfg["gamma"], v["n_step"])
            assert returns.dtype == np.float32
            np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
            # learn: dqn.py:167-188
            if v["freq"] > 0 and u % v["freq"] == 0:
                old.load_state_dict(net.state_dict())
            optim.zero_grad()
            qa = net(torch.as_tensor(store["obs"][idx]))[np.arange(len(idx)),
                                                         store["act"][idx]]
            ret = torch.as_tensor(returns).flatten()
            td = ret - qa
            if v["huber"]:
                loss = torch.nn.functional.huber_loss(qa.reshape(-1, 1), ret.reshape(-1, 1),
                                                      reduction="mean")
            else:
                w = torch.as_tensor(z[q + "weight"]) if v.get("per") else 1.0
                loss = (td.pow(2) * w).mean()
            loss.backward()
            optim.step()
            np.testing.assert_allclose(loss.item(), float(z[q + "loss"]), rtol=1e-6, err_msg=q)
            np.testing.assert_allclose(td.detach().numpy(), z[q + "td_error"], rtol=1e-6,
                                       atol=1e-6, err_msg=q)
            keys = param_keys(z, q + "param_")
            for (name, p), k in zip(sorted(net.state_dict().items()), keys):
                np.testing.assert_allclose(p.numpy(), z[k], rtol=1e-6, atol=1e-9,
                                           err_msg=f"{q}{name}")


def noise_host(act, eps, A, mask):
    """dqn.py:190-203 restated on NumPy's global stream."""
    bsz = len(act)
    rows = np.random.rand(bsz) < eps
    q = np.random.rand(bsz, A)
    if mask is not None:
        q += mask
    out = act.copy()
    out[rows] = q.argmax(axis=1)[rows]
    return out


def test_exploration_noise_cases_replay_bit_for_bit(z):
    cases = json.loads(str(z["noise_cfg"]))
    assert len(cases) == 12
    for i, c in enumerate(cases):
        p = f"noise{i}_"
        np.random.seed(c["seed"])
        got = noise_host(z[p + "act_in"], c["eps"], c["A"], z[p + "mask"] if c["masked"] else None)
        np.testing.assert_array_equal(got, z[p + "act_out"], err_msg=p)
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], z[p + "state_keys"], err_msg=p)
        assert st[2] == int(z[p + "state_pos"]), p
        if c["eps"] == 1.0:
            assert c["bsz"] == 1 or not np.array_equal(got, z[p + "act_in"])
        if c["masked"]:  # a masked-out action is never drawn
            changed = got != z[p + "act_in"]
            assert z[p + "mask"][np.arange(c["bsz"]), got][changed].all()
