from tianshou_amd.policy.base import BasePolicy
from tianshou_amd.policy.pg import PGPolicy
from tianshou_amd.policy.a2c import A2CPolicy
from tianshou_amd.policy.ppo import PPOPolicy
from tianshou_amd.policy.npg import NPGPolicy
from tianshou_amd.policy.trpo import TRPOPolicy
from tianshou_amd.policy.dqn import DQNPolicy
from tianshou_amd.policy.c51 import C51Policy
from tianshou_amd.policy.qrdqn import QRDQNPolicy
from tianshou_amd.policy.rainbow import RainbowPolicy
from tianshou_amd.policy.iqn import IQNPolicy
from tianshou_amd.policy.fqf import FQFPolicy
from tianshou_amd.policy.bdq import BranchingDQNPolicy
from tianshou_amd.policy.ddpg import DDPGPolicy
from tianshou_amd.policy.td3 import TD3Policy
from tianshou_amd.policy.sac import SACPolicy
from tianshou_amd.policy.discrete_sac import DiscreteSACPolicy
from tianshou_amd.policy.redq import REDQPolicy

__all__ = ["BasePolicy", "PGPolicy", "A2CPolicy", "PPOPolicy", "NPGPolicy", "TRPOPolicy",
           "DQNPolicy", "C51Policy", "QRDQNPolicy", "RainbowPolicy", "IQNPolicy", "FQFPolicy",
           "BranchingDQNPolicy", "DDPGPolicy", "TD3Policy", "SACPolicy", "DiscreteSACPolicy",
           "REDQPolicy"]
