"""BaseTrainer, OffpolicyTrainer and OnpolicyTrainer (tianshou/trainer/base.py:22-563): the
epoch iterator that drives a Collector, a policy and a test Collector.

One epoch collects ``step_per_epoch`` environment steps in chunks of ``step_per_collect``
steps or ``episode_per_collect`` episodes, updates the policy after every chunk and ends
with a test.  ``OffpolicyTrainer`` makes ``round(update_per_step * n/st)`` calls of
``policy.update(batch_size, buffer)`` per chunk -- on the device path each one is a fused
sample (``VectorReplayBuffer.sample_nstep``) and a graph replay; ``OnpolicyTrainer`` makes one
``policy.update(0, buffer, batch_size=, repeat=)`` over the whole buffer and resets it.

Not built: loggers beyond the no-op default (any object with the reference BaseLogger's
methods is accepted), ``resume_from_log``, OfflineTrainer and OffpolicyFullBufferTrainer.
"""
import time
from abc import ABC, abstractmethod
from collections import defaultdict, deque
from typing import Any, Callable, Dict, Optional, Tuple, Union

import numpy as np

from tianshou_amd.trainer.utils import gather_info, test_episode
from tianshou_amd.utils.statistics import MovAvg

try:
    import tqdm as _tqdm
except ImportError:  # the plain counter below prints nothing
    _tqdm = None


class NoopLogger:
    """The default logger: the reference BaseLogger's methods, doing nothing."""

    def log_train_data(self, collect_result: dict, step: int) -> None:
        pass

    log_test_data = log_update_data = log_train_data

    def save_data(self, epoch: int, env_step: int, gradient_step: int,
                  save_checkpoint_fn=None) -> None:
        pass

    def restore_data(self) -> Tuple[int, int, int]:
        return 0, 0, 0


class _Counter:
    """The part of a tqdm bar the epoch loop relies on (``n``, ``total``, ``update``,
    ``set_postfix``), silent."""

    def __init__(self, total: int, **kwargs: Any) -> None:
        self.total, self.n = total, 0

    def update(self, n: int = 1) -> None:
        self.n += n

    def set_postfix(self, **kwargs: Any) -> None:
        pass

    def __enter__(self) -> "_Counter":
        return self

    def __exit__(self, *exc: Any) -> None:
        pass


class BaseTrainer(ABC):
    """Iterator over epochs: every ``next()`` trains and tests one epoch and yields
    ``(epoch, epoch_stat, info)``; ``run()`` consumes it and returns the final ``info``
    (see :func:`~tianshou_amd.trainer.gather_info`).  Constructor arguments as
    tianshou/trainer/base.py:69-156."""

    def __init__(self, policy, max_epoch: int, batch_size: int, train_collector=None,
                 test_collector=None, buffer=None, step_per_epoch: Optional[int] = None,
                 repeat_per_collect: Optional[int] = None,
                 episode_per_test: Optional[int] = None, update_per_step: float = 1.0,
                 step_per_collect: Optional[int] = None,
                 episode_per_collect: Optional[int] = None,
                 train_fn: Optional[Callable[[int, int], None]] = None,
                 test_fn: Optional[Callable[[int, Optional[int]], None]] = None,
                 stop_fn: Optional[Callable[[float], bool]] = None,
                 save_best_fn: Optional[Callable[[Any], None]] = None,
                 save_checkpoint_fn: Optional[Callable[[int, int, int], str]] = None,
                 resume_from_log: bool = False,
                 reward_metric: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                 logger=None, verbose: bool = True, show_progress: bool = True,
                 test_in_train: bool = True) -> None:
        if resume_from_log:
            raise NotImplementedError("resume_from_log is not built")
        self.policy = policy
        self.buffer = buffer
        self.train_collector = train_collector
        self.test_collector = test_collector
        self.logger = logger if logger is not None else NoopLogger()
        self.start_time = time.time()
        self.stat = defaultdict(MovAvg)
        self.best_reward, self.best_reward_std = 0.0, 0.0
        self.start_epoch = 0
        self.gradient_step = 0
        self.env_step = 0
        self.max_epoch, self.step_per_epoch = max_epoch, step_per_epoch
        self.step_per_collect, self.episode_per_collect = step_per_collect, episode_per_collect
        self.update_per_step, self.repeat_per_collect = update_per_step, repeat_per_collect
        self.episode_per_test, self.batch_size = episode_per_test, batch_size
        self.train_fn, self.test_fn, self.stop_fn = train_fn, test_fn, stop_fn
        self.save_best_fn, self.save_checkpoint_fn = save_best_fn, save_checkpoint_fn
        self.reward_metric, self.verbose = reward_metric, verbose
        self.show_progress, self.test_in_train = show_progress, test_in_train
        self.is_run = False
        self.last_rew, self.last_len = 0.0, 0
        self.epoch = self.best_epoch = self.start_epoch
        self.stop_fn_flag = False
        self.iter_num = 0

    # -- iterator protocol ------------------------------------------------------------------------
    def reset(self) -> None:
        """Start over (base.py:215-260): counters and collector statistics to zero, the first
        test (epoch 0) sets the best reward, ``save_best_fn`` is called once."""
        self.is_run = False
        self.env_step = 0
        self.last_rew, self.last_len = 0.0, 0
        self.start_time = time.time()
        if self.train_collector is not None:
            self.train_collector.reset_stat()
            # testing in the middle of training needs the train collector to act with the
            # policy under training, and something to test on
            if self.train_collector.policy != self.policy or self.test_collector is None:
                self.test_in_train = False
        if self.test_collector is not None:
            assert self.episode_per_test is not None
            self.test_collector.reset_stat()
            first = test_episode(self.policy, self.test_collector, self.test_fn,
                                 self.start_epoch, self.episode_per_test, self.logger,
                                 self.env_step, self.reward_metric)
            self.best_epoch = self.start_epoch
            self.best_reward, self.best_reward_std = first["rew"], first["rew_std"]
        if self.save_best_fn:
            self.save_best_fn(self.policy)
        self.epoch = self.start_epoch
        self.stop_fn_flag = False
        self.iter_num = 0

    def __iter__(self) -> "BaseTrainer":
        self.reset()
        return self

    def _progress(self):
        if self.show_progress and _tqdm is not None:
            return _tqdm.tqdm(total=self.step_per_epoch, desc=f"Epoch #{self.epoch}",
                              dynamic_ncols=True, ascii=True)
        return _Counter(self.step_per_epoch)

    def __next__(self) -> Union[None, Tuple[int, Dict[str, Any], Dict[str, Any]]]:
        """One epoch, training then testing (base.py:266-350)."""
        self.epoch += 1
        self.iter_num += 1
        if self.iter_num > 1 and (self.epoch > self.max_epoch or self.stop_fn_flag):
            raise StopIteration
        self.policy.train()
        epoch_stat: Dict[str, Any] = {}
        result: Dict[str, Any] = {}
        with self._progress() as t:
            while t.n < t.total and not self.stop_fn_flag:
                data: Dict[str, Any] = {}
                result = {}
                if self.train_collector is not None:
                    data, result, self.stop_fn_flag = self.train_step()
                    t.update(result["n/st"])
                    if self.stop_fn_flag:  # stopped by the test in the middle of training
                        t.set_postfix(**data)
                        break
                else:
                    assert self.buffer, "No train_collector or buffer specified"
                    result["n/ep"] = len(self.buffer)
                    result["n/st"] = int(self.gradient_step)
                    t.update()
                self.policy_update_fn(data, result)
                t.set_postfix(**data)
            if t.n <= t.total and not self.stop_fn_flag:
                t.update()
        if self.train_collector is None:  # updates from a fixed buffer
            self.env_step = self.gradient_step * self.batch_size
        if not self.stop_fn_flag:
            self.logger.save_data(self.epoch, self.env_step, self.gradient_step,
                                  self.save_checkpoint_fn)
            if self.test_collector is not None:
                test_stat, self.stop_fn_flag = self.test_step()
                if not self.is_run:
                    epoch_stat.update(test_stat)
        if self.is_run:
            return None
        epoch_stat.update({k: v.get() for k, v in self.stat.items()})
        epoch_stat["gradient_step"] = self.gradient_step
        epoch_stat.update({"env_step": self.env_step, "rew": self.last_rew,
                           "len": int(self.last_len), "n/ep": int(result["n/ep"]),
                           "n/st": int(result["n/st"])})
        info = gather_info(self.start_time, self.train_collector, self.test_collector,
                           self.best_reward, self.best_reward_std)
        return self.epoch, epoch_stat, info

    # -- the two halves of an epoch ---------------------------------------------------------------
    def test_step(self) -> Tuple[Dict[str, Any], bool]:
        """The test at an epoch's end (base.py:352-394): best reward / epoch, save_best_fn on
        an improvement, stop_fn on the best reward."""
        assert self.episode_per_test is not None and self.test_collector is not None
        res = test_episode(self.policy, self.test_collector, self.test_fn, self.epoch,
                           self.episode_per_test, self.logger, self.env_step, self.reward_metric)
        rew, rew_std = res["rew"], res["rew_std"]
        if self.best_epoch < 0 or self.best_reward < rew:
            self.best_epoch = self.epoch
            self.best_reward = float(rew)
            self.best_reward_std = rew_std
            if self.save_best_fn:
                self.save_best_fn(self.policy)
        if self.verbose:
            print(f"Epoch #{self.epoch}: test_reward: {rew:.6f} ± {rew_std:.6f}, best_reward: "
                  f"{self.best_reward:.6f} ± {self.best_reward_std:.6f} in #{self.best_epoch}",
                  flush=True)
        test_stat = {} if self.is_run else {
            "test_reward": rew, "test_reward_std": rew_std, "best_reward": self.best_reward,
            "best_reward_std": self.best_reward_std, "best_epoch": self.best_epoch}
        stop = bool(self.stop_fn and self.stop_fn(self.best_reward))
        return test_stat, stop

    def train_step(self) -> Tuple[Dict[str, Any], Dict[str, Any], bool]:
        """One collect (base.py:396-439): train_fn, collect, env_step, and -- when episodes
        ended and stop_fn likes their reward -- a test in the middle of the epoch that can
        stop the run."""
        assert self.episode_per_test is not None and self.train_collector is not None
        stop = False
        if self.train_fn:
            self.train_fn(self.epoch, self.env_step)
        result = self.train_collector.collect(n_step=self.step_per_collect,
                                              n_episode=self.episode_per_collect)
        ended = result["n/ep"] > 0
        if ended and self.reward_metric:
            rew = self.reward_metric(result["rews"])
            result.update(rews=rew, rew=rew.mean(), rew_std=rew.std())
        self.env_step += int(result["n/st"])
        self.logger.log_train_data(result, self.env_step)
        if ended:
            self.last_rew, self.last_len = result["rew"], result["len"]
        data = {"env_step": str(self.env_step), "rew": f"{self.last_rew:.2f}",
                "len": str(int(self.last_len)), "n/ep": str(int(result["n/ep"])),
                "n/st": str(int(result["n/st"]))}
        if ended and self.test_in_train and self.stop_fn and self.stop_fn(result["rew"]):
            assert self.test_collector is not None
            res = test_episode(self.policy, self.test_collector, self.test_fn, self.epoch,
                               self.episode_per_test, self.logger, self.env_step)
            if self.stop_fn(res["rew"]):
                stop = True
                self.best_reward, self.best_reward_std = res["rew"], res["rew_std"]
            else:
                self.policy.train()
        return data, result, stop

    def log_update_data(self, data: Dict[str, Any], losses: Dict[str, Any]) -> None:
        """Moving averages of the losses (base.py:441-447): each loss replaced by the mean of
        its last 100 values, shown in the progress bar and handed to the logger."""
        for k in losses.keys():
            self.stat[k].add(losses[k])
            losses[k] = self.stat[k].get()
            data[k] = f"{losses[k]:.3f}"
        self.logger.log_update_data(losses, self.gradient_step)

    @abstractmethod
    def policy_update_fn(self, data: Dict[str, Any], result: Dict[str, Any]) -> None:
        """The updates after one collect (``data``: progress-bar fields, ``result``: the
        collect's result)."""

    def run(self) -> Dict[str, Union[float, str]]:
        """Consume the iterator; returns gather_info of the whole run (base.py:457-476)."""
        try:
            self.is_run = True
            deque(self, maxlen=0)
            info = gather_info(self.start_time, self.train_collector, self.test_collector,
                               self.best_reward, self.best_reward_std)
        finally:
            self.is_run = False
        return info

    # -- the two kinds of update -------------------------------------------------------------------
    def _sample_and_update(self, buffer, data: Dict[str, Any]) -> None:
        """One gradient step on one sampled minibatch (base.py:478-485)."""
        self.gradient_step += 1
        losses = self.policy.update(sample_size=self.batch_size, buffer=buffer)
        data.update({"gradient_step": str(self.gradient_step)})
        self.log_update_data(data, losses)

    def _update_on_entire_buffer(self, buffer, data: Dict[str, Any]) -> None:
        """learn() over the whole buffer in minibatches (base.py:487-507); gradient_step
        counts the minibatches of one pass."""
        losses = self.policy.update(sample_size=0, buffer=buffer, batch_size=self.batch_size,
                                    repeat=self.repeat_per_collect)
        self.gradient_step += 1 + (len(self.train_collector.buffer) - 0.1) // self.batch_size
        self.log_update_data(data, losses)


class OffpolicyTrainer(BaseTrainer):
    """``round(update_per_step * n/st)`` sampled updates after every collect
    (base.py:519-535)."""

    def policy_update_fn(self, data: Dict[str, Any], result: Dict[str, Any]) -> None:
        assert self.train_collector is not None
        for _ in range(round(self.update_per_step * result["n/st"])):
            self._sample_and_update(self.train_collector.buffer, data)


class OnpolicyTrainer(BaseTrainer):
    """One update over everything the collect stored, then an empty buffer
    (base.py:552-563)."""

    def policy_update_fn(self, data: Dict[str, Any], result: Optional[Dict[str, Any]] = None
                         ) -> None:
        assert self.train_collector is not None
        self._update_on_entire_buffer(self.train_collector.buffer, data)
        self.train_collector.reset_buffer(keep_statistics=True)


def offpolicy_trainer(*args: Any, **kwargs: Any) -> Dict[str, Union[float, str]]:
    """``OffpolicyTrainer(...).run()``."""
    return OffpolicyTrainer(*args, **kwargs).run()


def onpolicy_trainer(*args: Any, **kwargs: Any) -> Dict[str, Union[float, str]]:
    """``OnpolicyTrainer(...).run()``."""
    return OnpolicyTrainer(*args, **kwargs).run()
