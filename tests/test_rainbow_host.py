"""tests/golden/rainbow.npz (tools/gen_goldens.py gen_rainbow: the reference RainbowPolicy over
a dueling Net of NoisyLinear heads, on CPU torch) pinned on the host, and the CPU side of
utils/net.py's NoisyLinear / sample_noise / dueling Net and policy/rainbow.py's RainbowPolicy.

The replay runs this package's RainbowPolicy.learn with ``fused = False`` on CPU tensors over
batches rebuilt from the recorded sample indices, the recorded noise injected in place of the
sampler.  Tolerances are tests/test_dist_dqn_host.py's: n-step returns exact in f32 (the f64
n-step oracle, oracle/ref.py nstep_return, over the support), projected targets rtol 1e-6 /
atol 1e-9, losses rtol 1e-6, outgoing weights rtol 1e-6 / atol 1e-6, parameters rtol 1e-6 /
atol 1e-9 (autograd's own kernels against the reference's: same library, possibly another
summation split).  tests/test_gpu_rainbow.py compares the device policy with the same file."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref
from tests import test_dqn_host as dh
from tests.conftest import GOLDEN, ROOT

SYMBOLS = ("tsrl_noisy_eps", "tsrl_noisy_weights", "tsrl_noisy_grads", "tsrl_dueling_fwd",
           "tsrl_dueling_bwd")
EPS_KEYS = [f"{head}.model.{i}.eps_{pq}" for head in "QV" for i in (0, 2) for pq in "pq"]


@pytest.fixture(scope="module")
def z():
    return np.load(os.path.join(GOLDEN, "rainbow.npz"))


@pytest.fixture(scope="module")
def cfg(z):
    return json.loads(str(z["learn_cfg"]))


def make_net(cfg, device="cpu"):
    """The recorded network: Net(D, A, (16,), softmax, 51 atoms) with noisy Q / V heads."""
    from tianshou_amd.utils.net import Net, NoisyLinear
    head = {"hidden_sizes": tuple(cfg["head_hidden"]),
            "linear_layer": lambda x, y: NoisyLinear(x, y, cfg["noisy_std"])}
    return Net(cfg["D"], cfg["A"], hidden_sizes=tuple(cfg["hidden"]), device=device,
               softmax=True, num_atoms=cfg["c51"]["num_atoms"],
               dueling_param=(dict(head), dict(head)))


def init_state(z):
    return {k[len("init_"):]: torch.as_tensor(z[k]) for k in z.files if k.startswith("init_")}


def inject_noise(monkeypatch, z, policy, step):
    """Replace policy/rainbow.py's sampler: it copies the eps recorded for update ``step[0]``
    (a one-element list the caller advances) into the network it is called on."""
    from tianshou_amd.policy import rainbow as rb
    from tianshou_amd.utils.net import noisy_layers

    def recorded(model):
        which = "model" if model is policy.model else "old"
        sd = model.state_dict()
        with torch.no_grad():
            for k in EPS_KEYS:
                sd[k].copy_(torch.as_tensor(z[f"{step[1]}_u{step[0]}_eps_{which}_{k}"]))
        return bool(noisy_layers(model))

    monkeypatch.setattr(rb, "sample_noise", recorded)


def test_golden_is_pinned(z, cfg):
    assert set(cfg["variants"]) == {"target", "per", "rms", "notarget"}
    assert cfg["variants"]["target"]["freq"] == 2 and cfg["variants"]["target"]["optim"] == "adam"
    assert cfg["variants"]["per"]["per"] and cfg["variants"]["per"]["n_step"] == 3
    assert cfg["variants"]["rms"]["optim"] == "rms" and cfg["variants"]["notarget"]["freq"] == 0
    N, A, D = cfg["c51"]["num_atoms"], cfg["A"], cfg["D"]
    assert N == 51 and cfg["hidden"] == [16] and cfg["head_hidden"] == [16]
    shapes = {"model.model.0.weight": (16, D), "model.model.0.bias": (16,)}
    for head, out in (("Q", A * N), ("V", N)):
        for i, (fin, fout) in ((0, (16, 16)), (2, (16, out))):
            p = f"{head}.model.{i}."
            shapes.update({p + "mu_W": (fout, fin), p + "sigma_W": (fout, fin),
                           p + "mu_bias": (fout,), p + "sigma_bias": (fout,),
                           p + "eps_p": (fin,), p + "eps_q": (fout,)})
    init = init_state(z)
    assert {k: tuple(t.shape) for k, t in init.items()} == shapes
    params = {k: s for k, s in shapes.items() if ".eps_" not in k}
    for tag, v in cfg["variants"].items():
        assert float(z[tag + "_top2_gap"]) >= 1e-4, tag
        for u in range(6):
            q = f"{tag}_u{u}_"
            assert z[q + "indices"].shape == (v["bs"],) and z[q + "loss"].shape == ()
            assert z[q + "returns"].shape == z[q + "target_dist"].shape == (v["bs"], N)
            assert z[q + "out_weight"].shape == (v["bs"],)
            assert z[q + "returns"].dtype == z[q + "target_dist"].dtype == np.float32
            for which in ("model",) + (("old",) if v["freq"] else ()):
                for k in EPS_KEYS:
                    assert z[f"{q}eps_{which}_{k}"].shape == shapes[k], (q, which, k)
            assert (q + "eps_old_" + EPS_KEYS[0] in z.files) == bool(v["freq"])
            has = {k[len(q + "param_"):]: z[k].shape for k in z.files
                   if k.startswith(q + "param_")}
            assert has == (params if u in cfg["param_updates"][tag] else {}), q
            if v["freq"]:  # as sampled, ahead of any sync: the two networks' own draws
                assert not np.array_equal(z[f"{q}eps_old_{EPS_KEYS[0]}"],
                                          z[f"{q}eps_model_{EPS_KEYS[0]}"]), q
        assert 5 in cfg["param_updates"][tag]
        # an update that a later sync copies into the target is recorded
        if v["freq"]:
            assert {u - 1 for u in range(1, 6) if u % v["freq"] == 0} & \
                set(cfg["param_updates"][tag])
    assert "per_u5_leaves" in z.files and "per_max_prio" in z.files


def test_seeded_construction_equals_the_recording(z, cfg):
    from tianshou_amd.utils.net import Linear, NoisyLinear
    init = init_state(z)
    torch.manual_seed(cfg["init_seed"])
    net = make_net(cfg)
    sd = net.state_dict()
    assert list(sd) == list(init)  # the reference's keys in the reference's order
    for k, t in sd.items():
        assert torch.equal(t, init[k]), k
    assert net.output_dim == cfg["A"] * 51 and net.use_dueling
    # a bare layer after the trunk's Linear: the draws of Q's first layer
    torch.manual_seed(cfg["init_seed"])
    Linear(cfg["D"], 16)
    layer = NoisyLinear(16, 16, cfg["noisy_std"])
    assert set(layer.state_dict()) == {"mu_W", "sigma_W", "mu_bias", "sigma_bias", "eps_p",
                                       "eps_q"}
    for k, t in layer.state_dict().items():
        assert torch.equal(t, init["Q.model.0." + k]), k
    assert float(layer.sigma_W.detach()[0, 0]) == np.float32(0.5 / np.sqrt(16))
    # a plain Net is what it was: no heads, the same keys
    from tianshou_amd.utils.net import Net
    plain = Net(4, 2, hidden_sizes=(8,))
    assert plain.Q is None and plain.V is None and not plain.use_dueling
    assert list(plain.state_dict()) == ["model.model.0.weight", "model.model.0.bias",
                                        "model.model.2.weight", "model.model.2.bias"]


def test_sample_noise_and_forward_on_cpu(cfg):
    from tianshou_amd.utils.net import Net, NoisyLinear, sample_noise
    torch.manual_seed(3)
    net = make_net(cfg)
    assert sample_noise(net) is True
    assert sample_noise(Net(4, 2, hidden_sizes=(8,))) is False
    assert sample_noise(torch.nn.Linear(2, 2)) is False
    # sample(): the reference's two randn draws, eps_p first, through f
    layer = NoisyLinear(7, 5, 0.4)
    torch.manual_seed(21)
    layer.sample()
    torch.manual_seed(21)
    xp, xq = torch.randn(7), torch.randn(5)
    assert torch.equal(layer.eps_p, xp.sign() * xp.abs().sqrt())
    assert torch.equal(layer.eps_q, xq.sign() * xq.abs().sqrt())
    # sample_noise visits the layers in modules() order
    torch.manual_seed(22)
    sample_noise(net)
    torch.manual_seed(22)
    for head in (net.Q, net.V):
        for i in (0, 2):
            m = head.model[i]
            xp, xq = torch.randn(m.in_features), torch.randn(m.out_features)
            assert torch.equal(m.eps_p, xp.sign() * xp.abs().sqrt())
            assert torch.equal(m.eps_q, xq.sign() * xq.abs().sqrt())
    # training mode: mu + sigma * eps; eval mode: mu alone
    x = torch.randn(9, 7)
    w = layer.mu_W + layer.sigma_W * layer.eps_q.ger(layer.eps_p)
    b = layer.mu_bias + layer.sigma_bias * layer.eps_q
    assert layer.training and torch.equal(layer(x), torch.nn.functional.linear(x, w, b))
    layer.eval()
    assert torch.equal(layer(x), torch.nn.functional.linear(x, layer.mu_W, layer.mu_bias))
    assert not torch.equal(layer(x), torch.nn.functional.linear(x, w, b))
    # the effective parameters are no part of the state
    assert set(layer.state_dict()) == {"mu_W", "sigma_W", "mu_bias", "sigma_bias", "eps_p",
                                       "eps_q"}
    assert [n for n, _ in layer.named_parameters()] == ["mu_W", "sigma_W", "mu_bias",
                                                        "sigma_bias"]
    # the dueling Net on the CPU is common.py:273-284 as written
    obs = torch.randn(6, cfg["D"])
    out, state = net(obs, state="s")
    h = net.model(obs)
    q, v = net.Q(h).view(6, -1, 51), net.V(h).view(6, -1, 51)
    assert state == "s" and torch.equal(out, torch.softmax(q - q.mean(1, keepdim=True) + v, -1))
    # and without atoms: [b, A] values
    flat = Net(5, 3, hidden_sizes=(8,), dueling_param=({"hidden_sizes": (8,)},
                                                       {"hidden_sizes": (8,)}))
    obs = torch.randn(4, 5)
    h = flat.model(obs)
    q, v = flat.Q(h), flat.V(h)
    assert torch.equal(flat(obs)[0], q - q.mean(1, keepdim=True) + v)
    assert flat.output_dim == 3 and tuple(v.shape) == (4, 1)


def test_atari_rainbow_layout():
    from tianshou_amd.utils.net import Linear, NoisyLinear
    from tianshou_amd.utils.net_atari import DQN, Rainbow
    net = Rainbow(4, 84, 84, [6], num_atoms=51)
    assert isinstance(net, DQN) and net.output_dim == 6 * 51
    keys = list(net.state_dict())
    assert [k for k in keys if k.startswith("Q.")] == [
        f"Q.{i}.{n}" for i in (0, 2) for n in ("mu_W", "sigma_W", "mu_bias", "sigma_bias",
                                               "eps_p", "eps_q")]
    assert tuple(net.Q[0].mu_W.shape) == (512, 3136) and tuple(net.Q[2].mu_W.shape) == (306, 512)
    assert tuple(net.V[2].mu_W.shape) == (51, 512) and isinstance(net.V[0], NoisyLinear)
    plain = Rainbow(4, 84, 84, [6], num_atoms=51, is_dueling=False, is_noisy=False)
    assert not hasattr(plain, "V") and isinstance(plain.Q[0], Linear)
    obs = torch.randint(0, 256, (2, 4, 84, 84), dtype=torch.uint8)
    with torch.no_grad():
        out, _ = net(obs)
        feat, _ = DQN.forward(net, obs)
        q, v = net.Q(feat).view(-1, 6, 51), net.V(feat).view(-1, 1, 51)
    assert out.shape == (2, 6, 51)
    assert torch.equal(out, (q - q.mean(dim=1, keepdim=True) + v).softmax(dim=2))


@pytest.mark.parametrize("tag", ("target", "per", "rms", "notarget"))
def test_updates_replay_from_recorded_indices_and_noise(z, cfg, tag, monkeypatch):
    from tianshou_amd.data import Batch
    from tianshou_amd.policy import C51Policy, RainbowPolicy
    v = cfg["variants"][tag]
    vb, store = dh.host_buffer(z, cfg)
    np.testing.assert_array_equal(vb.sizes, z["buf_lengths"])
    np.testing.assert_array_equal(vb.last_index, z["buf_last_index"])
    net = make_net(cfg)
    net.load_state_dict(init_state(z))
    if v["optim"] == "rms":
        optim = torch.optim.RMSprop(net.parameters(), lr=7e-4, eps=1e-5, alpha=0.99)
    else:
        optim = torch.optim.Adam(net.parameters(), lr=1e-3)
    policy = RainbowPolicy(net, optim, **cfg["c51"], discount_factor=cfg["gamma"],
                           estimation_step=v["n_step"], target_update_freq=v["freq"])
    assert isinstance(policy, C51Policy) and policy.fused is True
    policy.fused = False
    assert not any(m.fused for m in net.modules() if hasattr(m, "eps_p"))
    step = [0, tag]
    inject_noise(monkeypatch, z, policy, step)
    forward, target_dist = policy.forward, policy._target_dist
    gaps, targets = [], []

    def rec_forward(batch, state=None, model="model", input="obs", **kw):
        res = forward(batch, state, model=model, input=input, **kw)
        if model == "model" and input == "obs_next":
            q64 = (res.logits.detach().double() * policy.support.double()).sum(2)
            gaps.append(dh_top2(q64.numpy()))
        return res

    def rec_target(batch):
        targets.append(target_dist(batch))
        return targets[-1]

    policy.forward, policy._target_dist = rec_forward, rec_target
    policy.train()
    support = policy.support.detach()
    for u in range(6):
        step[0] = u
        q = f"{tag}_u{u}_"
        idx = z[q + "indices"]
        terminal = idx % vb.maxsize
        for _ in range(v["n_step"] - 1):
            terminal = vb.next(terminal)
        returns, _ = ref.nstep_return(vb, store["terminated"], idx,
                                      support.repeat(len(idx), 1).numpy(), cfg["gamma"],
                                      v["n_step"])
        np.testing.assert_array_equal(returns, z[q + "returns"], err_msg=q)
        batch = Batch(obs=torch.as_tensor(store["obs"][idx]),
                      act=torch.as_tensor(store["act"][idx]),
                      obs_next=torch.as_tensor(store["obs_next"][idx]),
                      returns=torch.as_tensor(returns), info=Batch())
        if v.get("per"):
            batch.weight = torch.as_tensor(z[q + "weight"])
        res = policy.learn(batch)
        if v["freq"]:
            assert policy.model_old.training  # so that its noise takes effect
            synced = u % v["freq"] == 0
            for k in EPS_KEYS:  # a sync hands the online noise to the target
                same = torch.equal(policy.model_old.state_dict()[k], net.state_dict()[k])
                assert same == synced, (q, k)
        np.testing.assert_allclose(targets[u].numpy(), z[q + "target_dist"], rtol=1e-6,
                                   atol=1e-9, err_msg=q)
        np.testing.assert_allclose(res["loss"], float(z[q + "loss"]), rtol=1e-6, err_msg=q)
        np.testing.assert_allclose(batch.weight.numpy(), z[q + "out_weight"], rtol=1e-6,
                                   atol=1e-6, err_msg=q)
        if u in cfg["param_updates"][tag]:
            for k, t in net.state_dict().items():
                if ".eps_" not in k:
                    np.testing.assert_allclose(t.numpy(), z[q + "param_" + k], rtol=1e-6,
                                               atol=1e-9, err_msg=q + k)
    assert len(gaps) == 6
    np.testing.assert_allclose(min(gaps), float(z[tag + "_top2_gap"]), rtol=1e-3)
    assert policy._iter == 6 and policy._flat is None


def dh_top2(q):
    q = np.sort(np.asarray(q, np.float64), axis=1)
    best, second = q[:, -1], q[:, -2]
    return float(((best - second) / np.maximum(np.abs(best), np.abs(second))).min())


def test_new_symbols_are_declared_and_bound():
    from tianshou_amd import _C
    from tianshou_amd import policy as pol
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert name in _C.EXPORTED
        assert f" {name}(" in header
    assert f"#define TSRL_DUELING_MAX_ROW {_C.DUELING_MAX_ROW}\n" in header
    assert f"#define TSRL_ERR_DUELING_ROW {_C.ERR_DUELING_ROW}\n" in header
    assert "RainbowPolicy" in pol.__all__


def test_noisy_descriptor_matches_header(tmp_path):
    """tsrl_noisy_weights' device table is an int64 [n, NOISY_DESC_WORDS] tensor: the C struct
    is that many 8-byte fields, in and out last (a compiled probe)."""
    import subprocess
    from tianshou_amd import _C
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsrl.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(tsrl_noisy_layer), '
                   'offsetof(tsrl_noisy_layer, eps_p), offsetof(tsrl_noisy_layer, w_eff), '
                   'offsetof(tsrl_noisy_layer, in), offsetof(tsrl_noisy_layer, out));'
                   'return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert got == [8 * _C.NOISY_DESC_WORDS, 32, 48, 64, 72]
