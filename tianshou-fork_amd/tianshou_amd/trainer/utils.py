"""test_episode and gather_info (tianshou/trainer/utils.py:11-98)."""
import time
from typing import Any, Callable, Dict, Optional, Union

import numpy as np


def test_episode(policy, collector, test_fn: Optional[Callable[[int, Optional[int]], None]],
                 epoch: int, n_episode: int, logger=None, global_step: Optional[int] = None,
                 reward_metric: Optional[Callable[[np.ndarray], np.ndarray]] = None
                 ) -> Dict[str, Any]:
    """One evaluation: fresh envs and buffer, the policy in eval mode, ``test_fn(epoch,
    global_step)``, then ``n_episode`` episodes (utils.py:11-33)."""
    collector.reset_env()
    collector.reset_buffer()
    policy.eval()
    if test_fn:
        test_fn(epoch, global_step)
    result = collector.collect(n_episode=n_episode)
    if reward_metric:
        rew = reward_metric(result["rews"])
        result.update(rews=rew, rew=rew.mean(), rew_std=rew.std())
    if logger and global_step is not None:
        logger.log_test_data(result, global_step)
    return result


test_episode.__test__ = False  # a library function, not a pytest case


def gather_info(start_time: float, train_collector, test_collector, best_reward: float,
                best_reward_std: float) -> Dict[str, Union[float, str]]:
    """The counters and timings of a run (utils.py:36-98): ``train_step``,
    ``train_episode``, ``train_time/collector``, ``train_time/model``, ``train_speed``,
    ``test_step``, ``test_episode``, ``test_time``, ``test_speed``, ``best_reward``,
    ``best_result`` and ``duration``; the model time is what the collectors did not use."""
    duration = max(0, time.time() - start_time)
    model_time = duration
    info: Dict[str, Union[float, str]] = {"duration": f"{duration:.2f}s",
                                          "train_time/model": f"{model_time:.2f}s"}
    if test_collector is not None:
        test_time = test_collector.collect_time
        model_time = max(0, duration - test_time)
        info.update({
            "test_step": test_collector.collect_step,
            "test_episode": test_collector.collect_episode,
            "test_time": f"{test_time:.2f}s",
            "test_speed": f"{test_collector.collect_step / test_time:.2f} step/s",
            "best_reward": best_reward,
            "best_result": f"{best_reward:.2f} ± {best_reward_std:.2f}",
            "train_time/model": f"{model_time:.2f}s",
        })
    if train_collector is not None:
        train_window = duration - (test_collector.collect_time if test_collector is not None
                                   else 0.0)
        model_time = max(0, model_time - train_collector.collect_time)
        info.update({
            "train_step": train_collector.collect_step,
            "train_episode": train_collector.collect_episode,
            "train_time/collector": f"{train_collector.collect_time:.2f}s",
            "train_time/model": f"{model_time:.2f}s",
            "train_speed": f"{train_collector.collect_step / train_window:.2f} step/s",
        })
    return info
