"""The script that drives a trainer in tests/test_trainer_host.py and, with the reference's
trainers, in tools/gen_goldens.py gen_trainer_script: a collector and a policy that compute
nothing -- their collect results and losses come from seeded generators -- and write every call
made on them into one ordered log.  No device, no package import: the same objects serve both
trainer implementations."""
import numpy as np

HUGE = 1e9


class ScriptedBuffer:
    def __init__(self):
        self.rows = 0

    def __len__(self):
        return self.rows


class ScriptedPolicy:
    """train() / eval() / update() recorded; losses drawn from a seeded generator.  With
    ``repeat`` (the on-policy call) every loss is a list of ``repeat`` values."""

    def __init__(self, log, seed):
        self.log, self.rng = log, np.random.default_rng(seed)
        self.n_updates = 0
        self.training = True

    def train(self, mode=True):
        self.training = mode
        self.log.append(["policy", "train", {}])
        return self

    def eval(self):
        self.training = False
        self.log.append(["policy", "eval", {}])
        return self

    def update(self, sample_size, buffer, **kwargs):
        self.log.append(["policy", "update", dict(sample_size=sample_size, buffer=buffer.name,
                                                  buffer_len=len(buffer), **kwargs)])
        self.n_updates += 1
        repeat = kwargs.get("repeat")
        if repeat is None:
            out = {"loss": float(self.rng.normal(1.0, 0.3)),
                   "loss/aux": float(self.rng.normal(-2.0, 0.1))}
            if self.n_updates % 5 == 0:  # a value MovAvg has to leave out
                out["loss/aux"] = float("inf")
            return out
        return {"loss": [float(x) for x in self.rng.normal(1.0, 0.3, repeat)],
                "loss/clip": [float(x) for x in self.rng.normal(0.2, 0.05, repeat)]}


class ScriptedCollector:
    """collect() returns a result of the Collector's form.  Episode rewards rise with the
    number of updates the policy has had (``slope`` per update, from ``base``), so a stop_fn
    threshold is crossed at a known point of the script.  ``agents`` > 1: rewards of shape
    (episodes, agents), for a reward_metric."""

    def __init__(self, name, policy, log, seed, base=0.0, slope=0.05, agents=1):
        self.name, self.policy, self.log = name, policy, log
        self.rng = np.random.default_rng(seed)
        self.base, self.slope, self.agents = base, slope, agents
        self.buffer = ScriptedBuffer()
        self.buffer.name = name + "_buffer"
        self.collect_step = self.collect_episode = 0
        self.collect_time = 0.0

    def reset_stat(self):
        self.log.append([self.name, "reset_stat", {}])
        self.collect_step = self.collect_episode = 0
        self.collect_time = 0.0

    def reset_env(self):
        self.log.append([self.name, "reset_env", {}])

    def reset_buffer(self, keep_statistics=False):
        self.log.append([self.name, "reset_buffer", dict(keep_statistics=keep_statistics)])
        self.buffer.rows = 0

    def collect(self, n_step=None, n_episode=None):
        self.log.append([self.name, "collect", dict(n_step=n_step, n_episode=n_episode)])
        rng = self.rng
        if n_episode is not None:
            lens = rng.integers(3, 9, n_episode)
            n_st = int(lens.sum())
        else:
            n_st = int(n_step)
            lens = rng.integers(3, 9, int(rng.integers(0, 3)))
        n_ep = len(lens)
        shape = (n_ep,) if self.agents == 1 else (n_ep, self.agents)
        rews = self.base + self.slope * self.policy.n_updates + rng.normal(0.0, 0.02, shape)
        self.collect_step += n_st
        self.collect_episode += n_ep
        self.collect_time += 0.001 * n_st
        self.buffer.rows += n_st
        if n_ep > 0:
            rew, rew_std = rews.mean(), rews.std()
            ln, ln_std = lens.mean(), lens.std()
        else:
            rew = rew_std = ln = ln_std = 0
        return {"n/ep": n_ep, "n/st": n_st, "rews": rews, "lens": lens,
                "idxs": np.arange(n_ep), "rew": rew, "len": ln, "rew_std": rew_std,
                "len_std": ln_std}


# name -> (trainer kind, constructor keywords, script options).  stop_at: the stop_fn
# threshold; test_base: where the test collector's rewards start relative to the train
# collector's (below it: a train reward can cross the threshold before the test reward does).
COMMON = dict(max_epoch=3, batch_size=16, episode_per_test=4, step_per_epoch=32)
VARIANTS = {
    "off_ups1": ("off", dict(COMMON, step_per_collect=8, update_per_step=1.0), {}),
    "off_ups025": ("off", dict(COMMON, step_per_collect=10, update_per_step=0.25), {}),
    "off_ups25": ("off", dict(COMMON, step_per_collect=5, update_per_step=2.5), {}),
    "off_episode": ("off", dict(COMMON, episode_per_collect=3, update_per_step=0.5), {}),
    "off_stop_in_train": ("off", dict(COMMON, step_per_collect=4, update_per_step=1.0,
                                      test_in_train=True),
                          dict(stop_at=1.6, test_base=-0.5)),
    "off_stop_at_test": ("off", dict(COMMON, step_per_collect=8, update_per_step=1.0,
                                     test_in_train=False), dict(stop_at=2.0)),
    "off_no_test": ("off", dict(COMMON, step_per_collect=8, update_per_step=1.0),
                    dict(no_test=True)),
    "off_metric": ("off", dict(COMMON, step_per_collect=8, update_per_step=1.0),
                   dict(agents=2)),
    "on_steps": ("on", dict(COMMON, step_per_collect=16, repeat_per_collect=2), {}),
    "on_episode": ("on", dict(COMMON, episode_per_collect=2, repeat_per_collect=3),
                   dict(stop_at=HUGE)),
}


def build(name):
    """(trainer kind, constructor keywords with the scripted objects and recording hooks,
    the log) of one variant."""
    kind, kw, opt = VARIANTS[name]
    log = []
    policy = ScriptedPolicy(log, seed=1)
    agents = opt.get("agents", 1)
    train = ScriptedCollector("train", policy, log, seed=2, agents=agents)
    test = None if opt.get("no_test") else ScriptedCollector(
        "test", policy, log, seed=3, base=opt.get("test_base", 0.0), agents=agents)
    stop_at = opt.get("stop_at", HUGE)

    def train_fn(epoch, env_step):
        log.append(["hook", "train_fn", dict(epoch=epoch, env_step=env_step)])

    def test_fn(epoch, env_step):
        log.append(["hook", "test_fn", dict(epoch=epoch, env_step=env_step)])

    def stop_fn(mean_rewards):
        log.append(["hook", "stop_fn", dict(mean_rewards=float(mean_rewards))])
        return bool(mean_rewards >= stop_at)

    def save_best_fn(p):
        log.append(["hook", "save_best_fn", dict(policy=p is policy)])

    def reward_metric(rews):
        log.append(["hook", "reward_metric", dict(shape=list(np.shape(rews)))])
        return rews[:, 0] * 0.75 + rews[:, 1] * 0.25

    kw = dict(kw, policy=policy, train_collector=train, test_collector=test, train_fn=train_fn,
              test_fn=test_fn, stop_fn=stop_fn, save_best_fn=save_best_fn, verbose=False,
              show_progress=False)
    if agents > 1:
        kw["reward_metric"] = reward_metric
    return kind, kw, log


def plain(x):
    """JSON form of a stat / info / log value, keeping int and float apart."""
    if isinstance(x, dict):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    return x


TIMED = ("duration", "train_time/model", "train_time/collector", "train_speed", "test_time",
         "test_speed")


def drive(trainer_cls, kw):
    """Iterate one trainer to its end: [(epoch, stat, info)] in JSON form, time fields left
    out, and the trainer."""
    trainer = trainer_cls(**kw)
    epochs = []
    for epoch, stat, info in trainer:
        epochs.append(dict(epoch=epoch, stat=plain(stat),
                           info=plain({k: v for k, v in info.items() if k not in TIMED})))
    return epochs, trainer
