from tianshou_amd.trainer.base import (BaseTrainer, NoopLogger, OfflineTrainer,
                                       OffpolicyTrainer, OnpolicyTrainer, offline_trainer,
                                       offpolicy_trainer, onpolicy_trainer)
from tianshou_amd.trainer.utils import gather_info, test_episode

__all__ = ["BaseTrainer", "OfflineTrainer", "OffpolicyTrainer", "OnpolicyTrainer",
           "offline_trainer", "offpolicy_trainer", "onpolicy_trainer", "test_episode",
           "gather_info", "NoopLogger"]
