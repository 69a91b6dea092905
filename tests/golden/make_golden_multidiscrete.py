"""Golden vectors for the MultiDiscrete actor head and flat action masks, from the REFERENCE ITSELF.

The reference's ActorCritic with its MultiDiscreteActorHead (rl_algo_impls/shared/actor/multi_discrete.py) or
its CategoricalActorHead under a flat mask (shared/actor/categorical.py MaskedCategorical), stepped by its own
PPO.learn_epoch and A2C.learn over fixed minibatches with num_actions=None, through the stubs of make_golden.py:

  md          obs Box(5,), act MultiDiscrete([3, 5, 2]), hidden [64, 64], tanh, no masks; PPO
  md_masked   the same space, hidden [20], relu, masks; A2C
  cat_masked  obs Box(5,), act Discrete(6), hidden [64, 64], tanh, masks; PPO
  md_w1       act MultiDiscrete([3, 1, 4]) (a group of width 1), hidden [20], tanh, masks; forward only

Masks (case_inputs): entries valid with probability 0.65, every group of a row repaired to keep one valid entry,
then row 0 fully valid, row 1 with exactly ONE valid entry in its widest group, row 2 with its first group ALL
FALSE (the reference's float32 result there: normalised logits 0, so log-prob 0, entropy 0, no gradient).
Actions are drawn among the valid entries (any entry in an all-false group).

Per case: the state_dict key names and shapes; forward(obs, actions, masks) at B = 7 and B = 130 (logp, entropy,
v) and the gradients of sum(w1 logp + w2 entropy + w3 v) for fixed random w; three optimizer steps on fixed
minibatches (parameters, loss and pre-clip gradient norm after each).  Everything is also run by the same
reference modules in float64 from the same bits, and max |f32 - f64| per quantity is stored (over the batch for
logp / entropy / v, per tensor for gradients and parameters): the reference's own rounding, the yardstick of the
tests.  The maximum, not the element's own difference: one element's |f32 - f64| is a single draw of the
rounding error and can be near zero by chance (a value head output that nearly cancels), where it bounds
nothing; the maximum over the batch is the scale of the reference's rounding for that quantity, the same rule as
the per-tensor maxima of the gradients and the per-quantity maxima of the kernel tests.

Initial weights: the PCG64 recipe of make_golden_pong.pong_init.

    python tests/golden/make_golden_multidiscrete.py            # writes multidiscrete_steps.npz
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden_pong import INIT_SEED, pong_init  # noqa: E402

FWD_B = (7, 130)
OBS_DIM = 5
CASES = {
    "md": dict(algo="ppo", n=3, B=64, nvec=[3, 5, 2], masked=False, seed=41,
               policy=dict(pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64], activation_fn="tanh"),
               kw=dict(learning_rate=3e-4, batch_size=64, clip_range=0.2, ent_coef=0.01, vf_coef=0.5)),
    "md_masked": dict(algo="a2c", n=3, B=40, nvec=[3, 5, 2], masked=True, seed=43,
                      policy=dict(pi_hidden_sizes=[20], v_hidden_sizes=[20], activation_fn="relu"),
                      kw=dict(learning_rate=7e-4, ent_coef=0.01, vf_coef=0.5)),
    "cat_masked": dict(algo="ppo", n=3, B=64, nvec=None, n_act=6, masked=True, seed=47,
                       policy=dict(pi_hidden_sizes=[64, 64], v_hidden_sizes=[64, 64], activation_fn="tanh"),
                       kw=dict(learning_rate=3e-4, batch_size=64, clip_range=0.2, ent_coef=0.01, vf_coef=0.5)),
    "md_w1": dict(algo=None, n=0, B=0, nvec=[3, 1, 4], masked=True, seed=53,
                  policy=dict(pi_hidden_sizes=[20], v_hidden_sizes=[20], activation_fn="tanh"), kw={}),
}


def groups_of(case) -> list:
    return list(case["nvec"]) if case["nvec"] is not None else [case["n_act"]]


def masks_and_actions(rng, n: int, groups: list, masked: bool):
    """(masks (n, A) bool | None, actions (n, G) int64) of one batch; see the module docstring."""
    A, off = int(np.sum(groups)), np.concatenate([[0], np.cumsum(groups)])
    mask = rng.random((n, A)) < 0.65
    for g, w in enumerate(groups):  # one valid entry per group at least
        keep = rng.integers(0, w, size=n)
        empty = ~mask[:, off[g]:off[g + 1]].any(axis=1)
        mask[np.nonzero(empty)[0], off[g] + keep[empty]] = True
    if n >= 3:
        mask[0] = True
        wide = int(np.argmax(groups))
        mask[1, off[wide]:off[wide + 1]] = False
        mask[1, off[wide] + groups[wide] // 2] = True
        mask[2, off[0]:off[1]] = False
    if not masked:
        mask[:] = True
    actions = np.zeros((n, len(groups)), np.int64)
    for i in range(n):
        for g, w in enumerate(groups):
            valid = np.nonzero(mask[i, off[g]:off[g + 1]])[0]
            actions[i, g] = rng.choice(valid) if len(valid) else rng.integers(0, w)
    return (mask if masked else None), actions


def case_inputs(case: dict):
    """The fixed inputs of a case (numpy only): forward batches with their loss weights, and the update's
    minibatch obs / actions / masks / noise terms (the old log-probs and values are the policy's own plus
    noise).  Discrete actions are (n,), MultiDiscrete (n, G)."""
    rng = np.random.default_rng(case["seed"])
    groups = groups_of(case)

    def batch(n):
        obs = rng.standard_normal((n, OBS_DIM)).astype(np.float32)
        mask, act = masks_and_actions(rng, n, groups, case["masked"])
        return obs, (act if case["nvec"] is not None else act[:, 0]), mask

    fwd = {}
    for B in FWD_B:
        obs, act, mask = batch(B)
        fwd[B] = dict(obs=obs, actions=act, masks=mask, w=rng.standard_normal((B, 3)).astype(np.float32))
    upd = []
    for _ in range(case["n"]):
        obs, act, mask = batch(case["B"])
        upd.append(dict(obs=obs, actions=act, masks=mask,
                        d_logp=(rng.standard_normal(case["B"]) * 0.1).astype(np.float32),
                        d_v=(rng.standard_normal(case["B"]) * 0.2).astype(np.float32),
                        advantages=(rng.standard_normal(case["B"]) * 2).astype(np.float32)))
    return fwd, upd


def load_flat(policy, flat: np.ndarray) -> None:
    off = 0
    with torch.no_grad():
        for p in policy.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(flat[off:off + n]).reshape(p.shape).to(p.dtype))
            off += n


def flat64(ts) -> np.ndarray:
    return torch.cat([t.detach().reshape(-1).double() for t in ts]).numpy().copy()


def make_policy(mg, case):
    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    act = gs.MultiDiscrete(np.array(case["nvec"])) if case["nvec"] is not None else gs.Discrete(case["n_act"])
    env = mg.StubVecEnv(1, gs.Box(-np.inf, np.inf, (OBS_DIM,), np.float32), act)
    torch.manual_seed(7)
    return ActorCritic(env, **case["policy"])


def run_case(mg, name, case, f64: bool, init, batches_f32=None):
    from rl_algo_impls.a2c import a2c as a2c_mod
    from rl_algo_impls.rollout.rollout import Batch
    from rl_algo_impls.shared.callbacks.summary_wrapper import SummaryWrapper

    policy = make_policy(mg, case)
    sd_keys = [[k, list(v.shape)] for k, v in policy.state_dict().items()]
    if f64:
        policy = policy.double()
        policy.network._feature_extractor.preprocess = lambda obs: obs.double()  # the flat encoder's obs.float()
    load_flat(policy, init)
    dt = torch.float64 if f64 else torch.float32
    T = lambda a: torch.from_numpy(a).to(dt)
    M = lambda m: None if m is None else torch.from_numpy(m)
    I = lambda a: torch.from_numpy(a)
    fwd_in, upd_in = case_inputs(case)
    rec = dict(state_dict=sd_keys, fwd={}, batches=[])
    for B, d in fwd_in.items():
        policy.zero_grad(set_to_none=True)
        lp, ent, v = policy(T(d["obs"]), I(d["actions"]), action_masks=M(d["masks"]))
        w = T(d["w"])
        (w[:, 0] * lp + w[:, 1] * ent + w[:, 2] * v).sum().backward()
        rec["fwd"][B] = dict(logp=flat64([lp]), entropy=flat64([ent]), v=flat64([v]),
                             grads=flat64([p.grad for p in policy.parameters()]))
    policy.zero_grad(set_to_none=True)
    if case["n"] == 0:
        return rec, [tuple(p.shape) for p in policy.parameters()]
    # the update's minibatches: made once by the f32 policy, shared (as the same bits) with the f64 run
    if batches_f32 is None:
        batches_f32 = []
        with torch.no_grad():
            for d in upd_in:
                lp, _, v = policy(T(d["obs"]), I(d["actions"]), action_masks=M(d["masks"]))
                values = (v + T(d["d_v"])).float().numpy()
                b = dict(obs=d["obs"], actions=d["actions"], logprobs=(lp + T(d["d_logp"])).float().numpy(),
                         values=values, advantages=d["advantages"], returns=(values + d["advantages"]).astype(np.float32))
                if d["masks"] is not None:
                    b["masks"] = d["masks"]
                batches_f32.append(b)
    rec["batches"] = batches_f32
    ppo = case["algo"] == "ppo"
    batches = [Batch(T(b["obs"]), T(b["logprobs"]) if ppo else None, I(b["actions"]), M(b.get("masks")), None,
                     T(b["values"]), T(b["advantages"]), T(b["returns"])) for b in batches_f32]
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
    return rec, [tuple(p.shape) for p in policy.parameters()]


def main():
    import make_golden as mg  # imports the reference with its stubs

    arrays, index = {}, dict(init_seed=INIT_SEED, torch=torch.__version__, numpy=np.__version__, fwd_B=list(FWD_B))
    for name, case in CASES.items():
        shapes = [tuple(p.shape) for p in make_policy(mg, case).parameters()]
        init = pong_init(shapes)
        rec, _ = run_case(mg, name, case, False, init)
        rec64, _ = run_case(mg, name, case, True, init, rec["batches"])
        cut = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        pmax = lambda v: np.array([np.abs(v[cut[j]:cut[j + 1]]).max() for j in range(len(shapes))], np.float32)
        up32 = lambda e: np.nextafter(np.asarray(e, np.float32), np.float32(np.inf))  # never round an error down
        P = f"{name}_"
        for B in FWD_B:
            d, f, f6 = case_inputs(case)[0][B], rec["fwd"][B], rec64["fwd"][B]
            arrays[f"{P}fwd{B}_obs"], arrays[f"{P}fwd{B}_actions"], arrays[f"{P}fwd{B}_w"] = d["obs"], d["actions"], d["w"]
            if d["masks"] is not None:
                arrays[f"{P}fwd{B}_masks"] = d["masks"]
            for k in ("logp", "entropy", "v"):
                arrays[f"{P}fwd{B}_{k}"] = f[k].astype(np.float32)
                arrays[f"{P}fwd{B}_err_{k}"] = up32(np.abs(f[k] - f6[k]).max())
            arrays[f"{P}fwd{B}_grads"] = f["grads"].astype(np.float32)
            arrays[f"{P}fwd{B}_err_grads"] = up32(pmax(f["grads"] - f6["grads"]))
        index[name] = dict(case, shapes=[list(s) for s in shapes], state_dict=rec["state_dict"], obs_dim=OBS_DIM)
        line = (f"{name}: P={cut[-1]} |f32 - f64|: logp {arrays[f'{P}fwd130_err_logp'].max():.3e} entropy "
                f"{arrays[f'{P}fwd130_err_entropy'].max():.3e} grads {arrays[f'{P}fwd130_err_grads'].max():.3e}")
        if case["n"]:
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
            line += (f" params {arrays[P + 'err_params'].max():.3e} loss {arrays[P + 'err_loss'].max():.3e} norms "
                     f"{arrays[P + 'err_norms'].max():.3e}\n  loss={arrays[P + 'loss']} norms={arrays[P + 'norms']}")
        print(line)
    arrays["index"] = np.array(json.dumps(index))
    np.savez_compressed(HERE / "multidiscrete_steps.npz", **arrays)
    print("wrote multidiscrete_steps.npz", (HERE / "multidiscrete_steps.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
