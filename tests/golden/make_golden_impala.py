"""Golden vectors for the IMPALA CNN encoder (cnn_style: impala), from the REFERENCE ITSELF.

The reference's ActorCritic with its ImpalaCnn encoder (rl_algo_impls/shared/encoder/impala_cnn.py:11-92,
`/range_size` prescale cnn.py:24-27; procgen's policy hyperparameters, rl_algo_impls/hyperparams/
ppo.yml:433-438) on a small non-square frame, uint8 3x20x12 (after the three pools 20 -> 10 -> 5 -> 3 and
12 -> 6 -> 3 -> 2: odd sizes), Categorical(15), stepped by the reference's own PPO.learn_epoch over three
fixed minibatches of 32 rows with procgen's clip_range 0.2, clip_range_vf 0.2, ent_coef 0.01, lr 5e-4
(ppo.yml:441-450).

Initial weights: the PCG64 recipe of make_golden_pong.pong_init (host independent).

The same update is also run by the same reference module in float64 from the same bits (the only change:
the prescale casts to float64 instead of float32), and the per-quantity |f32 - f64| is stored: the
reference's own rounding, the yardstick of the GPU tests' tolerances (for the final parameters: per
tensor, the maximum over its elements).

    python tests/golden/make_golden_impala.py      # writes impala_steps.npz
"""
from __future__ import annotations

import copy
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden_pong import INIT_SEED, pong_init  # noqa: E402

OBS_SHAPE = (3, 20, 12)
N_ACTIONS = 15
POLICY_KW = dict(activation_fn="relu", cnn_style="impala", cnn_flatten_dim=256)


def main():
    import make_golden as mg  # imports the reference with its stubs
    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.ppo.ppo import PPO
    from rl_algo_impls.rollout.rollout import Batch
    from rl_algo_impls.shared.encoder import cnn as cnn_mod
    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    kw = dict(learning_rate=5e-4, batch_size=32, clip_range=0.2, clip_range_vf=0.2, vf_coef=0.5, ent_coef=0.01)
    n_batches, B = 3, 32
    env = mg.StubVecEnv(1, gs.Box(0, 255, OBS_SHAPE, np.uint8), gs.Discrete(N_ACTIONS), kind="pong")
    torch.manual_seed(7)
    policy = ActorCritic(env, **POLICY_KW)
    sd_keys = [[k, list(v.shape)] for k, v in policy.state_dict().items()]
    shapes = [tuple(p.shape) for p in policy.parameters()]
    init = pong_init(shapes)
    off = 0
    with torch.no_grad():
        for p in policy.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(init[off:off + n]).reshape(p.shape))
            off += n
    rng = np.random.default_rng(17)
    batches = [mg.make_batch(policy, B, rng, OBS_SHAPE, discrete_n=N_ACTIONS, obs_u8=True) for _ in range(n_batches)]
    with torch.no_grad():
        fwd0 = policy(batches[0].obs, batches[0].actions)
    policy64 = copy.deepcopy(policy).double()

    rec = mg.run_reference_update(PPO, policy, batches, kw)

    # float64: the same module, the same bits; the prescale's cast follows the module's dtype
    real_pre = cnn_mod.CnnEncoder.preprocess

    def preprocess64(self, obs):
        if len(obs.shape) == 3:
            obs = obs.unsqueeze(0)
        return obs.double() / self.range_size

    cnn_mod.CnnEncoder.preprocess = preprocess64
    try:
        b64 = [Batch(b.obs, b.logprobs.double(), b.actions, None, None, b.values.double(), b.advantages.double(),
                     b.returns.double()) for b in batches]
        with torch.no_grad():
            fwd0_64 = policy64(b64[0].obs, b64[0].actions)
        rec64 = run_update_f64(mg, PPO, policy64, b64, kw)
    finally:
        cnn_mod.CnnEncoder.preprocess = real_pre

    arrays = {}
    for i, b in enumerate(batches):
        for f in ("obs", "logprobs", "actions", "values", "advantages", "returns"):
            arrays[f"b{i}_{f}"] = getattr(b, f).numpy()
    sizes = [int(np.prod(s)) for s in shapes]
    cut = np.cumsum([0] + sizes)
    per = lambda v: np.array([np.sqrt(np.sum(np.square(np.asarray(v[cut[j]:cut[j + 1]], np.float64))))
                              for j in range(len(sizes))])
    stats = mg.stats_array(rec["stats"], 1)
    stats64 = mg.stats_array(rec64["stats"], 1)
    arrays["norms"] = np.array(rec["norms"], np.float64)
    arrays["stats"] = stats
    arrays["params"] = rec["params"][-1]
    arrays["step1_param_delta_norms"] = per(rec["params"][0] - init)
    arrays["grads1_norms"] = per(rec["grads"][0])
    arrays["opt_state1_norms"] = per(rec["opt_state1"])
    arrays["opt_state2_norms"] = per(rec["opt_state2"])
    for name, t in zip(("logp", "entropy", "v"), fwd0):
        arrays[f"fwd0_{name}"] = t.numpy()
    # the float64 run and the reference's own float32 rounding against it
    arrays["f64_norms"] = np.array(rec64["norms"], np.float64)
    arrays["f64_stats"] = stats64
    arrays["f64_param_norms"] = per(rec64["params"][-1])
    arrays["f64_grads1_norms"] = per(rec64["grads"][0])
    arrays["f64_opt_state1_norms"] = per(rec64["opt_state1"])
    for name, t in zip(("logp", "entropy", "v"), fwd0_64):
        arrays[f"f64_fwd0_{name}"] = t.numpy()
    arrays["err_norms"] = np.abs(arrays["norms"] - arrays["f64_norms"])
    arrays["err_stats"] = np.abs(stats - stats64)
    # (the float64 parameter vector itself would double the file: its per-tensor norms and the per-tensor
    # maximum of |f32 - f64| are kept)
    perr = np.abs(arrays["params"].astype(np.float64) - rec64["params"][-1])
    arrays["err_params"] = np.array([perr[cut[j]:cut[j + 1]].max() for j in range(len(sizes))])
    # the fraction of weights on which the two runs disagree about "moved by more than lr / 2" (the
    # check of test_gpu_pong.py:118-121)
    lr = kw["learning_rate"]
    moved32 = np.abs(arrays["params"] - init) > 0.5 * lr
    moved64 = np.abs(rec64["params"][-1] - init.astype(np.float64)) > 0.5 * lr
    arrays["err_moved_fraction"] = np.array(float((moved32 != moved64).mean()))
    # per-tensor norms of the whole update's displacement (final parameters - init) in both precisions
    arrays["param_delta_norms"] = per(arrays["params"] - init)
    arrays["f64_param_delta_norms"] = per(rec64["params"][-1] - init.astype(np.float64))
    arrays["err_param_delta_norms"] = np.abs(arrays["param_delta_norms"] - arrays["f64_param_delta_norms"])
    arrays["err_grads1_norms"] = np.abs(arrays["grads1_norms"] - arrays["f64_grads1_norms"])
    arrays["err_opt_state1_norms"] = np.abs(arrays["opt_state1_norms"] - arrays["f64_opt_state1_norms"])
    for name in ("logp", "entropy", "v"):
        arrays[f"err_fwd0_{name}"] = np.abs(arrays[f"fwd0_{name}"].astype(np.float64) - arrays[f"f64_fwd0_{name}"])
    index = dict(kw=kw, n=n_batches, B=B, shapes=[list(s) for s in shapes], state_dict=sd_keys,
                 init_seed=INIT_SEED, opt_step=rec["opt_step"], torch=torch.__version__, numpy=np.__version__,
                 policy=POLICY_KW, obs_shape=list(OBS_SHAPE), n_actions=N_ACTIONS)
    arrays["index"] = np.array(json.dumps(index))
    np.savez_compressed(HERE / "impala_steps.npz", **arrays)
    print(f"impala_steps.npz: {n_batches} x {B} rows, P={cut[-1]}, norms={arrays['norms']}")
    print(f"  |f32 - f64|: norms {arrays['err_norms']}, params max {arrays['err_params'].max():.3e}, "
          f"stats max {arrays['err_stats'].max():.3e}")


def run_update_f64(mg, PPO, policy, batches, kw):
    """make_golden.run_reference_update keeping float64 (its flat() casts to float32)."""
    real_flat = mg.flat
    mg.flat = lambda ts: torch.cat([t.detach().reshape(-1).double() for t in ts]).numpy().copy()
    try:
        return mg.run_reference_update(PPO, policy, batches, kw)
    finally:
        mg.flat = real_flat


if __name__ == "__main__":
    main()
