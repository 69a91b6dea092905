"""Golden vectors for the gSDE actor head (use_sde, squash_output), from the REFERENCE ITSELF.

The reference's ActorCritic with its StateDependentNoiseActorHead
(rl_algo_impls/shared/actor/state_dependent_noise.py), stepped by its own PPO.learn_epoch and A2C.learn
over fixed minibatches, through the stubs of make_golden.py:

  full    obs Box(5,), act Box(3,), hidden [64, 64], tanh, full_std, no squash, log_std_init -2; PPO
  squash  obs Box(5,), act Box(3,), hidden [20], relu, full_std=False, squash_output; A2C.  Its actions
          are tanh(x) with |x| <= 2, so TanhBijector's clamp never binds and the float64 rerun (whose
          clamp uses the float64 epsilon) stays comparable.

Per case: the state_dict key names and shapes; forward(obs, actions) at B = 7 and B = 130 (logp, entropy,
v) and the gradients of sum(w1 logp + w2 entropy + w3 v) for fixed random w; three optimizer steps on
fixed minibatches (parameters, loss and pre-clip gradient norm after each).  Everything is also run by
the same reference modules in float64 from the same bits, and |f32 - f64| per quantity is stored (per
tensor for gradients and parameters): the reference's own rounding, the yardstick of the tests.

Initial weights: the PCG64 recipe of make_golden_pong.pong_init, then log_std = log_std_init + 0.25 z
with z from the same kind of stream (sde_init below; a constant log_std would hide an (h, a) mix-up).

    python tests/golden/make_golden_sde.py            # writes sde_steps.npz
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

FWD_B = (7, 130)
CASES = {
    "full": dict(algo="ppo", n=3, B=64,
                 policy=dict(pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64], activation_fn="tanh", use_sde=True,
                             full_std=True, squash_output=False, log_std_init=-2.0),
                 kw=dict(learning_rate=3e-4, batch_size=64, clip_range=0.2, ent_coef=0.01, vf_coef=0.5)),
    "squash": dict(algo="a2c", n=3, B=40,
                   policy=dict(pi_hidden_sizes=[20], v_hidden_sizes=[20], activation_fn="relu", use_sde=True,
                               full_std=False, squash_output=True, log_std_init=-1.0),
                   kw=dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.5)),
}
OBS_DIM, ACT_DIM = 5, 3


def sde_init(shapes, log_std_index: int, log_std_init: float, seed: int = INIT_SEED) -> np.ndarray:
    """Flat f32 initial parameters in parameters() order: pong_init, with the log_std tensor replaced by
    log_std_init + 0.25 * N(0, 1) from PCG64(seed + 1).  Numpy only: the tests regenerate the same bits."""
    flat = pong_init([tuple(s) for s in shapes], seed)
    sizes = [int(np.prod(s)) for s in shapes]
    off = int(np.sum(sizes[:log_std_index]))
    z = np.random.default_rng(seed + 1).standard_normal(sizes[log_std_index]).astype(np.float32)
    flat[off:off + sizes[log_std_index]] = np.float32(log_std_init) + np.float32(0.25) * z
    return flat


def load_flat(policy, flat: np.ndarray) -> None:
    off = 0
    with torch.no_grad():
        for p in policy.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(flat[off:off + n]).reshape(p.shape).to(p.dtype))
            off += n


def flat64(ts) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1).double() for t in ts]).numpy().copy()


def case_inputs(name: str, case: dict):
    """The fixed inputs of a case (numpy only): forward batches with their loss weights, and the update's
    minibatch obs / actions / noise terms (the old log-probs and values are the policy's own plus noise)."""
    rng = np.random.default_rng(29 if name == "full" else 31)
    squash = case["policy"]["squash_output"]

    def obs_act(n):
        obs = rng.standard_normal((n, OBS_DIM)).astype(np.float32)
        if squash:
            act = np.tanh(np.clip(rng.standard_normal((n, ACT_DIM)) * 0.7, -2.0, 2.0)).astype(np.float32)
        else:
            act = (rng.standard_normal((n, ACT_DIM)) * 0.5).astype(np.float32)
        return obs, act

    fwd = {}
    for B in FWD_B:
        obs, act = obs_act(B)
        fwd[B] = dict(obs=obs, actions=act, w=rng.standard_normal((B, 3)).astype(np.float32))
    upd = []
    for _ in range(case["n"]):
        obs, act = obs_act(case["B"])
        upd.append(dict(obs=obs, actions=act, d_logp=(rng.standard_normal(case["B"]) * 0.1).astype(np.float32),
                        d_v=(rng.standard_normal(case["B"]) * 0.2).astype(np.float32),
                        advantages=(rng.standard_normal(case["B"]) * 2).astype(np.float32)))
    return fwd, upd


def run_case(mg, name, case, f64: bool, init, batches_f32=None):
    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.a2c import a2c as a2c_mod
    from rl_algo_impls.rollout.rollout import Batch
    from rl_algo_impls.shared.callbacks.summary_wrapper import SummaryWrapper
    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    env = mg.StubVecEnv(1, gs.Box(-np.inf, np.inf, (OBS_DIM,), np.float32), gs.Box(-1.0, 1.0, (ACT_DIM,), np.float32),
                        kind="halfcheetah")
    torch.manual_seed(7)
    policy = ActorCritic(env, **case["policy"])
    sd_keys = [[k, list(v.shape)] for k, v in policy.state_dict().items()]
    if f64:
        policy = policy.double()
        policy.network._feature_extractor.preprocess = lambda obs: obs.double()  # the flat encoder's obs.float()
    load_flat(policy, init)
    dt = torch.float64 if f64 else torch.float32
    T = lambda a: torch.from_numpy(a).to(dt)
    fwd_in, upd_in = case_inputs(name, case)
    rec = dict(state_dict=sd_keys, fwd={}, batches=[])
    for B, d in fwd_in.items():
        policy.zero_grad(set_to_none=True)
        lp, ent, v = policy(T(d["obs"]), T(d["actions"]))
        w = T(d["w"])
        (w[:, 0] * lp + w[:, 1] * ent + w[:, 2] * v).sum().backward()
        rec["fwd"][B] = dict(logp=flat64([lp]), entropy=flat64([ent]), v=flat64([v]),
                             grads=flat64([p.grad for p in policy.parameters()]))
    policy.zero_grad(set_to_none=True)
    # the update's minibatches: made once by the f32 policy, shared (as the same bits) with the f64 run
    if batches_f32 is None:
        batches_f32 = []
        with torch.no_grad():
            for d in upd_in:
                lp, _, v = policy(T(d["obs"]), T(d["actions"]))
                values = (v + T(d["d_v"])).float().numpy()
                batches_f32.append(dict(obs=d["obs"], actions=d["actions"], logprobs=(lp + T(d["d_logp"])).float().numpy(),
                                        values=values, advantages=d["advantages"],
                                        returns=(values + d["advantages"]).astype(np.float32)))
    rec["batches"] = batches_f32
    ppo = case["algo"] == "ppo"
    batches = [Batch(T(b["obs"]), T(b["logprobs"]) if ppo else None, T(b["actions"]), None, None, T(b["values"]),
                     T(b["advantages"]), T(b["returns"])) for b in batches_f32]
    tbw = SummaryWrapper(mg.SummaryWriter())
    if ppo:
        algo = mg.PPO(policy, torch.device("cpu"), tbw, n_epochs=1, **case["kw"])
    else:
        algo = mg.A2C(policy, torch.device("cpu"), tbw, **case["kw"])
    rec.update(params=[], norms=[], loss=[])
    orig = algo.optimizer_step

    def optimizer_step():
        g = flat64([p.grad if p.grad is not None else torch.zeros_like(p) for p in policy.parameters()])
        rec["norms"].append(float(np.sqrt(np.sum(g * g))))  # the pre-clip norm clip_grad_norm_ computes
        out = orig()
        rec["params"].append(flat64(policy.parameters()))
        return out

    algo.optimizer_step = optimizer_step
    mod = mg.ppo_mod if ppo else a2c_mod
    real_tss = mod.TrainStepStats

    def tss(*args):
        rec["loss"].append(float(args[0]))
        return real_tss(*args)

    mod.TrainStepStats = tss
    try:
        if ppo:  # one epoch over the n fixed minibatches: n optimizer steps
            r = mg.FixedRollout(batches)
            algo.learn_epoch(0, r.total_steps, mg.FixedGen(r), None)
        else:  # A2C takes one optimizer step per rollout: n rollouts of one minibatch each
            rollouts = iter([mg.FixedRollout([b]) for b in batches])

            class Gen:
                vec_env = None

                def rollout(self, gamma, gae_lambda):
                    return next(rollouts)

            algo.learn(sum(len(b) for b in batches), Gen())
    finally:
        mod.TrainStepStats = real_tss
    assert len(rec["params"]) == len(rec["loss"]) == case["n"]
    return rec, [tuple(p.shape) for p in policy.parameters()], [k for k, _ in policy.named_parameters()]


def main():
    import make_golden as mg  # imports the reference with its stubs

    arrays, index = {}, dict(init_seed=INIT_SEED, torch=torch.__version__, numpy=np.__version__, fwd_B=list(FWD_B))
    for name, case in CASES.items():
        # shapes and the log_std index first (a throw-away policy), then the two runs from the same bits
        shapes, names = probe(mg, case)
        ls_index = names.index("network._pi.log_std")
        init = sde_init(shapes, ls_index, case["policy"]["log_std_init"])
        rec, _, _ = run_case(mg, name, case, False, init)
        rec64, _, _ = run_case(mg, name, case, True, init, rec["batches"])
        cut = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        pmax = lambda v: np.array([np.abs(v[cut[j]:cut[j + 1]]).max() for j in range(len(shapes))], np.float32)
        up32 = lambda e: np.nextafter(np.asarray(e, np.float32), np.float32(np.inf))  # never round an error down
        P = f"{name}_"
        for B in FWD_B:
            d, f, f6 = case_inputs(name, case)[0][B], rec["fwd"][B], rec64["fwd"][B]
            arrays[f"{P}fwd{B}_obs"], arrays[f"{P}fwd{B}_actions"], arrays[f"{P}fwd{B}_w"] = d["obs"], d["actions"], d["w"]
            for k in ("logp", "entropy", "v"):
                arrays[f"{P}fwd{B}_{k}"] = f[k].astype(np.float32)
                arrays[f"{P}fwd{B}_err_{k}"] = up32(np.abs(f[k] - f6[k]))
            arrays[f"{P}fwd{B}_grads"] = f["grads"].astype(np.float32)
            arrays[f"{P}fwd{B}_err_grads"] = up32(pmax(f["grads"] - f6["grads"]))
        for i, b in enumerate(rec["batches"]):
            for k, v in b.items():
                if k != "logprobs" or case["algo"] == "ppo":
                    arrays[f"{P}b{i}_{k}"] = v
        arrays[P + "params"] = np.stack(rec["params"]).astype(np.float32)
        arrays[P + "err_params"] = up32(np.stack([pmax(a - b) for a, b in zip(rec["params"], rec64["params"])]))
        arrays[P + "loss"] = np.array(rec["loss"])
        arrays[P + "err_loss"] = np.abs(np.array(rec["loss"]) - np.array(rec64["loss"]))
        arrays[P + "norms"] = np.array(rec["norms"])
        arrays[P + "err_norms"] = np.abs(np.array(rec["norms"]) - np.array(rec64["norms"]))
        index[name] = dict(case, shapes=[list(s) for s in shapes], state_dict=rec["state_dict"], log_std_index=ls_index,
                           obs_dim=OBS_DIM, act_dim=ACT_DIM)
        print(f"{name}: P={cut[-1]} loss={arrays[P + 'loss']} norms={arrays[P + 'norms']}")
        print(f"  |f32 - f64|: logp {arrays[f'{P}fwd130_err_logp'].max():.3e} entropy "
              f"{arrays[f'{P}fwd130_err_entropy'].max():.3e} grads {arrays[f'{P}fwd130_err_grads'].max():.3e} "
              f"params {arrays[P + 'err_params'].max():.3e} loss {arrays[P + 'err_loss'].max():.3e} "
              f"norms {arrays[P + 'err_norms'].max():.3e}")
    arrays["index"] = np.array(json.dumps(index))
    np.savez_compressed(HERE / "sde_steps.npz", **arrays)
    print("wrote sde_steps.npz", (HERE / "sde_steps.npz").stat().st_size, "bytes")


def probe(mg, case):
    """(parameter shapes, parameter names) of the case's reference policy."""
    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    env = mg.StubVecEnv(1, gs.Box(-np.inf, np.inf, (OBS_DIM,), np.float32), gs.Box(-1.0, 1.0, (ACT_DIM,), np.float32),
                        kind="halfcheetah")
    policy = ActorCritic(env, **case["policy"])
    return [tuple(p.shape) for p in policy.parameters()], [k for k, _ in policy.named_parameters()]


if __name__ == "__main__":
    main()
