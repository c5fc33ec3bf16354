from tianshou_amd.trainer.base import (BaseTrainer, NoopLogger, OffpolicyTrainer,
                                       OnpolicyTrainer, offpolicy_trainer, onpolicy_trainer)
from tianshou_amd.trainer.utils import gather_info, test_episode

__all__ = ["BaseTrainer", "OffpolicyTrainer", "OnpolicyTrainer", "offpolicy_trainer",
           "onpolicy_trainer", "test_episode", "gather_info", "NoopLogger"]
