"""tianshou_amd.trainer against the reference's trainers, without a device: both are driven by
the scripted collector and policy of tests/trainer_script.py, and tests/golden/
trainer_script.npz (tools/gen_goldens.py gen_trainer_script) holds what the reference's
OffpolicyTrainer / OnpolicyTrainer did with them -- the ordered call log (object, method,
keyword arguments), every epoch's (stat, info) and the final state, for update_per_step 1.0 /
0.25 / 2.5 (round() to even), step_per_collect and episode_per_collect, a stop_fn that fires in
the middle of an epoch (after one middle test that did not pass) and one that fires at an
epoch's test, a missing test collector, a reward_metric, and the hooks.  The generator asserts
that the reference run reaches each of those branches.

Integers (and which values are integers) must agree exactly, floats to rel 1e-12; the log
exactly.  Also here: MovAvg, the silent progress counter, and the C ABI of the fused sample."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import trainer_script as ts
from tests.conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "trainer_script.npz")) as f:
        return json.loads(str(f["data"]))


def _classes():
    from tianshou_amd.trainer import OffpolicyTrainer, OnpolicyTrainer
    return {"off": OffpolicyTrainer, "on": OnpolicyTrainer}


def _same(got, want, where):
    """Nested comparison: same keys, same kinds, ints (and bools, strings) exactly, floats to
    rel 1e-12."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), where
        for k in want:
            _same(got[k], want[k], f"{where}[{k!r}]")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    elif isinstance(want, float):
        assert isinstance(got, float), (where, type(got))
        assert got == pytest.approx(want, rel=1e-12, abs=0.0), where
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


def test_golden_covers_every_variant(golden):
    assert list(golden) == list(ts.VARIANTS)


@pytest.mark.parametrize("name", list(ts.VARIANTS))
def test_iteration_matches_reference(golden, name, capsys):
    want = golden[name]
    kind, kw, log = ts.build(name)
    epochs, tr = ts.drive(_classes()[kind], kw)
    assert ts.plain(log) == want["log"], name  # object, method, keyword arguments, in order
    assert len(epochs) == len(want["epochs"])
    for g, w in zip(epochs, want["epochs"]):
        _same(g, w, f"{name} epoch {w['epoch']}")
    final = ts.plain(dict(epoch=tr.epoch, env_step=tr.env_step, gradient_step=tr.gradient_step,
                          best_epoch=tr.best_epoch, best_reward=tr.best_reward,
                          best_reward_std=tr.best_reward_std, stop_fn_flag=tr.stop_fn_flag))
    _same(final, want["final"], name + " final")
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""  # verbose=False, show_progress=False: silent


@pytest.mark.parametrize("name", list(ts.VARIANTS))
def test_run_matches_reference(golden, name):
    want = golden[name]
    kind, kw, log = ts.build(name)
    trainer = _classes()[kind](**kw)
    info = trainer.run()
    assert not trainer.is_run
    assert ts.plain(log) == want["run_log"], name
    _same(ts.plain({k: v for k, v in info.items() if k not in ts.TIMED}), want["run"],
          name + " run()")
    for k in ts.TIMED:  # the time fields exist where the reference has them
        assert (k in info) == (k.startswith("test_") is False or kw["test_collector"] is not None)


def test_wrappers_run_the_trainers(golden):
    from tianshou_amd.trainer import offpolicy_trainer, onpolicy_trainer
    for name, fn in (("off_ups025", offpolicy_trainer), ("on_steps", onpolicy_trainer)):
        _, kw, log = ts.build(name)
        info = fn(**kw)
        assert ts.plain(log) == golden[name]["run_log"]
        assert info["best_reward"] == pytest.approx(golden[name]["run"]["best_reward"],
                                                    rel=1e-12)


def test_epoch_stat_carries_moving_average_losses(golden):
    """The stat of an epoch holds every loss key as the mean of its last 100 finite values;
    the script's infinite loss/aux values are left out of it."""
    kind, kw, log = ts.build("off_ups1")
    epochs, tr = ts.drive(_classes()[kind], kw)
    stat = epochs[-1]["stat"]
    assert {"loss", "loss/aux", "gradient_step", "env_step", "rew", "len", "n/ep", "n/st",
            "test_reward", "test_reward_std", "best_reward", "best_reward_std",
            "best_epoch"} == set(stat)
    assert np.isfinite(stat["loss/aux"]) and len(tr.stat["loss/aux"].cache) == 96 - 96 // 5
    assert len(tr.stat["loss"].cache) == 96


def test_default_logger_and_progress_bar(capsys):
    """No logger given: the no-op one.  show_progress=True draws a bar on stderr only (tqdm
    where it imports); nothing goes to stdout with verbose=False."""
    from tianshou_amd.trainer import NoopLogger, OffpolicyTrainer
    _, kw, _ = ts.build("off_ups025")
    tr = OffpolicyTrainer(**dict(kw, show_progress=True, max_epoch=1))
    assert isinstance(tr.logger, NoopLogger)
    assert len(list(tr)) == 1
    assert capsys.readouterr().out == ""
    with pytest.raises(NotImplementedError):
        OffpolicyTrainer(**dict(kw, resume_from_log=True))


def test_logger_receives_the_reference_calls():
    from tianshou_amd.trainer import OffpolicyTrainer
    _, kw, _ = ts.build("off_ups025")
    seen = []

    class Logger:
        def log_train_data(self, res, step):
            seen.append(("train", step))

        def log_test_data(self, res, step):
            seen.append(("test", step))

        def log_update_data(self, res, step):
            seen.append(("update", step, sorted(res)))

        def save_data(self, epoch, env_step, gradient_step, fn):
            seen.append(("save", epoch, env_step, gradient_step, fn))

    OffpolicyTrainer(**dict(kw, logger=Logger(), max_epoch=1)).run()
    assert seen[0] == ("test", 0) and seen[1] == ("train", 10)
    assert seen[2] == ("update", 1, ["loss", "loss/aux"]) and seen[3][:2] == ("update", 2)
    assert seen[-2] == ("save", 1, 40, 8, None) and seen[-1] == ("test", 40)


def test_movavg():
    import torch
    from tianshou_amd.utils import MovAvg
    m = MovAvg(size=4)
    assert m.get() == 0.0 and m.std() == 0.0
    assert m.add(torch.tensor(5)) == 5.0
    assert m.add(float("inf")) == 5.0 and m.add(float("nan")) == 5.0 and m.add(-np.inf) == 5.0
    assert m.add([6, 7, 8]) == 6.5 and m.mean() == 6.5
    assert m.std() == pytest.approx(np.std([5, 6, 7, 8]))
    assert m.add(np.array([1.0, 2.0])) == np.mean([7, 8, 1, 2])  # the last four
    assert MovAvg(0).add(list(range(200))) == np.mean(range(200))  # size 0: unbounded


# -- the C ABI of the fused sample -----------------------------------------------------------------
def test_replay_sample_abi_is_declared_and_exported():
    from tianshou_amd import _C
    lib = ctypes.CDLL(_C.LIB_PATH)
    with open(os.path.join(ROOT, "include", "tsrl.h")) as f:
        header = f.read()
    for name in ("tsrl_replay_sample", "tsrl_nstep_apply"):
        assert name in _C.EXPORTED and hasattr(lib, name)
        assert f"int {name}(" in header


def test_replay_sample_args_layout(tmp_path):
    """tsrl_replay_sample_args: the ctypes mirror has the C struct's size and offsets."""
    from tianshou_amd import _C
    fields = [f for f, _ in _C.ReplaySampleArgs._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsrl.h"\nint main(){'
                   'printf("%zu", sizeof(tsrl_replay_sample_args));'
                   + "".join(f'printf(" %zu", offsetof(tsrl_replay_sample_args, {f}));'
                             for f in fields) + "}")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert out[0] == ctypes.sizeof(_C.ReplaySampleArgs)
    assert out[1:] == [getattr(_C.ReplaySampleArgs, f).offset for f in fields]
