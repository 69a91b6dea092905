"""Plugin registries under the reference's names (rl_algo_impls/runner/running_utils.py:38-55),
so `--algo ppo|a2c|acbc|dqn` hyperparameters resolve to the MI355X implementations.

ALGOS is the on-policy set over the rollout + GAE hot path, every member of which runs on
SyncStepRolloutGenerator (tests/test_boundary.py pins exactly that).  The off-policy DQN is registered in
OFF_POLICY_ALGOS; ALL_ALGOS is the union, the table to merge into the reference's own ALGOS.  POLICIES and
DEFAULT_ROLLOUT_GENERATORS carry every algorithm of ALL_ALGOS."""
from __future__ import annotations

from .a2c import A2C
from .acbc import ACBC
from .dqn import DQN, DQNPolicy
from .policy import ActorCritic
from .ppo import PPO
from .reference_rollout import ReferenceAIRolloutGenerator
from .replay import ReplayBufferRolloutGenerator
from .rollout import SyncStepRolloutGenerator

ALGOS = {"ppo": PPO, "a2c": A2C, "acbc": ACBC}
OFF_POLICY_ALGOS = {"dqn": DQN}
ALL_ALGOS = {**ALGOS, **OFF_POLICY_ALGOS}
POLICIES = {"ppo": ActorCritic, "a2c": ActorCritic, "acbc": ActorCritic, "dqn": DQNPolicy}
DEFAULT_ROLLOUT_GENERATORS = {"ppo": SyncStepRolloutGenerator, "a2c": SyncStepRolloutGenerator,
                              "acbc": SyncStepRolloutGenerator, "dqn": ReplayBufferRolloutGenerator}
# the keys of rl_algo_impls/runner/train.py's rollout_type switch that are built here (guided and
# guided_random are not)
ROLLOUT_GENERATORS = {"sync": SyncStepRolloutGenerator, "reference": ReferenceAIRolloutGenerator}
