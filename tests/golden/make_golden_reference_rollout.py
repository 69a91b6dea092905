"""Golden rollout of the reference's own ReferenceAIRolloutGenerator
(rl_algo_impls/rollout/reference_ai_rollout.py), imported with ./stubs as make_golden.py does.  Data only:
the env script (reference_rollout.npz: obs, masks, last_action, rewards, dones for T = 6, N = 3 on a 4x4 map,
recorded from rl_algo_impls_amd.envs.ScriptedBotGridVecEnv, the rewards spread over the three critics'
columns), the state_dict of a small squeeze-U-Net policy with three critics (POLICY_KW below), and
the resulting VecRollout's fields (include_logp=False, as every reference YAML sets).

    python tests/golden/make_golden_reference_rollout.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))
T, N, HW = 6, 3, (4, 4)
# make_golden_squnet.py's small policy has the C5 structure (three levels, strides [[2, 2], [2, 2]] with growing
# down-conv kernels), whose decoder does not line up on a 4x4 map (the reference itself fails there: 4 against 16
# columns), so this policy keeps what the rollout can see of it -- K = 3 critics (tanh, identity), the
# subaction_mask, critic_channels 16 -- on two levels and one stride
POLICY_KW = dict(actor_head_style="squeeze_unet", channels_per_level=[8, 16], strides_per_level=[2],
                 encoder_residual_blocks_per_level=[1, 1], critic_channels=16,
                 additional_critic_activation_functions=["tanh", "identity"],
                 subaction_mask={0: {1: 1, 2: 2, 3: 3, 4: 4, 5: 4, 6: 5}})
GAMMA, GAE_LAMBDA = np.array([0.99, 0.999, 0.999]), np.array([0.95, 0.99, 0.99])  # ppo-Microrts.yml, per critic


def record_script():
    """The script the replaying envs follow: T + 1 observation / mask batches, T steps' results."""
    import _pkgload

    _pkgload.load()
    from rl_algo_impls_amd.envs import ScriptedBotGridVecEnv

    env = ScriptedBotGridVecEnv(N, map_hw=HW, seed=21, term_prob=0.25)
    obs, _ = env.reset()
    s = dict(obs=[obs.copy()], masks=[env.get_action_mask().copy()], last_action=[], rewards=[], dones=[])
    for _ in range(T):
        obs, rew, term, trunc, _ = env.step(np.zeros((N, 16, 7), dtype=np.int64))
        s["obs"].append(obs.copy())
        s["masks"].append(env.get_action_mask().copy())
        s["last_action"].append(env.last_action.copy())
        s["rewards"].append(np.stack([rew, 0.5 - rew, np.float32(0.25) * rew], axis=-1))  # one column per critic
        s["dones"].append(term | trunc)
    return {k: np.stack(v) for k, v in s.items()}


def main():
    script = record_script()
    import make_golden as mg

    mg.import_reference()
    from gymnasium.spaces import Box, MultiDiscrete
    from rl_algo_impls.rollout.reference_ai_rollout import ReferenceAIRolloutGenerator
    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    nvec = np.array([6, 4, 4, 4, 4, 7, 49], dtype=np.int64)

    class ReplayEnv:
        """Replays the script through the reference's VectorEnv calls."""

        num_envs = N
        single_observation_space = Box(low=0.0, high=1.0, shape=(7,) + HW, dtype=np.float32)
        single_action_space = MultiDiscrete(np.tile(nvec, 16))
        action_plane_space = MultiDiscrete(nvec)

        def __init__(self):
            self.t = 0
            self.received = []

        @property
        def unwrapped(self):
            return self

        def reset(self, **kw):
            return script["obs"][0], {}

        def get_action_mask(self):
            return script["masks"][self.t]

        def step(self, actions):
            self.received.append(np.array(actions))
            t = self.t
            self.last_action = script["last_action"][t]
            self.t += 1
            return script["obs"][t + 1], script["rewards"][t], script["dones"][t], {}

    env = ReplayEnv()
    torch.manual_seed(9)
    policy = ActorCritic(env, **POLICY_KW).to(torch.device("cpu"))
    out = {f"script_{k}": v for k, v in script.items()}
    for k, v in policy.state_dict().items():
        out[f"init/{k}"] = v.detach().numpy().copy()
    gen = ReferenceAIRolloutGenerator(policy, env, n_steps=T, include_logp=False,
                                      subaction_mask=POLICY_KW["subaction_mask"])
    r = gen.rollout(gamma=GAMMA, gae_lambda=GAE_LAMBDA)
    assert r.logprobs is None and all(not a.any() for a in env.received)
    for f in ("obs", "actions", "rewards", "episode_starts", "values", "action_masks", "advantages", "returns"):
        out[f"rollout_{f}"] = np.asarray(getattr(r, f))
    out["rollout_next_episode_starts"] = np.asarray(gen.next_episode_starts)
    out["gamma"], out["gae_lambda"] = GAMMA, GAE_LAMBDA
    np.savez_compressed(HERE / "reference_rollout.npz", **out)
    print("wrote", HERE / "reference_rollout.npz", {k: v.shape for k, v in out.items() if k.startswith("rollout_")})


if __name__ == "__main__":
    main()
