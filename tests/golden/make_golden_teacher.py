"""Golden vectors for PPO's teacher-KL loss term, from the REFERENCE ITSELF (run on the CPU).

Loss-level cases (`L<i>_*`): the reference's TeacherKLLoss (rl_algo_impls/loss/teacher_kl_loss.py) inside
the PPO minibatch loss of rl_algo_impls/ppo/ppo.py:307-374, written out here as one torch expression over
given network outputs (new_logp, entropy, new_values as leaves), differentiated by autograd:

  B in {5, 300, 2049}  x  unbiased in {True, False}  x  importance sampling in {True, False}
  x  (K = 1 | K = 2 with multi_reward_weights [0.7, 0.3]; at B = 2049, K = 2 the default variant only, to
  keep the file under the repository's size limit),
  and at B = 300, K = 1, the default variant: kl_cutoff tripped (pi_coef = 0; the teacher term stays),
  gradient_accumulation's 1/3 scale, clip_range_vf = 0.2.

Inputs: t - l uniform in [-3, 3] with every 7th row t == l exactly; l - o ~ N(0, 0.1), every 5th row
+-[0.3, 0.7] (ratios outside the clip range).  Recorded: d loss / d new_logp, d loss / d new_values, the loss,
the un-scaled teacher term, pi_loss, approx_kl.

Step-level cases (`cat_*`, `md_masked_*`): the reference's PPO.learn_epoch (2 epochs, batch 16 over
T = 5 x N = 8 rows: minibatches 16 / 16 / 8, fixed permutations) with TeacherKLLoss over a stub
checkpoints holder whose teacher is a second initialisation of the same architecture; default
unbiased / importance-sampling options, teacher_kl_loss_coef 2e-2:

  cat         obs Box(4,), Discrete(2), hidden [8, 8], tanh
  md_masked   obs Box(5,), MultiDiscrete([3, 5, 2]), hidden [8, 8], tanh, flat masks (the teacher's forward
              receives them: the masks of make_golden_multidiscrete.masks_and_actions)

Recorded per optimizer step: loss, teacher_kl_loss, pre-clip gradient norm, parameters; and the
teacher_logprobs field the reference's add_to_batch made (chunks of num_envs = 8 rows).

Everything is run in float32 and, from the same bits, in float64.  The float64 result is the record
(`<name>`), the float32 one is kept next to it (`<name>_f32`), and `<name>_err` is max |f32 - f64| (over
the batch; per tensor for parameters): the reference's own rounding, the yardstick of the tests.

    python tests/golden/make_golden_teacher.py            # writes teacher_kl_steps.npz
"""
from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from make_golden_multidiscrete import flat64, load_flat, masks_and_actions  # noqa: E402
from make_golden_pong import pong_init  # noqa: E402

COEF = 2e-2
T_STEPS, N_ENVS, BATCH, EPOCHS = 5, 8, 16, 2
STEP_CASES = {
    "cat": dict(obs_dim=4, nvec=None, n_act=2, masked=False, seed=61,
                policy=dict(pi_hidden_sizes=[8, 8], v_hidden_sizes=[8, 8], activation_fn="tanh"),
                kw=dict(learning_rate=3e-4, batch_size=BATCH, n_epochs=EPOCHS, clip_range=0.2, ent_coef=0.01,
                        vf_coef=0.5, teacher_kl_loss_coef=COEF)),
    "md_masked": dict(obs_dim=5, nvec=[3, 5, 2], n_act=None, masked=True, seed=67,
                      policy=dict(pi_hidden_sizes=[8, 8], v_hidden_sizes=[8, 8], activation_fn="tanh"),
                      kw=dict(learning_rate=3e-4, batch_size=BATCH, n_epochs=EPOCHS, clip_range=0.2, ent_coef=0.01,
                              vf_coef=0.5, teacher_kl_loss_coef=COEF)),
}
MRW = [0.7, 0.3]


def loss_cases() -> list:
    cases = []
    for B, K, (unb, imp) in itertools.product((5, 300, 2049), (1, 2), itertools.product((True, False), repeat=2)):
        if B == 2049 and K == 2 and not (unb and imp):  # (the file's size: one K = 2 case at the largest B)
            continue
        cases.append(dict(B=B, K=K, unbiased=unb, importance_sampling=imp, coef=COEF, kl_cutoff=None,
                          grad_scale=1.0, clip_range_vf=None))
    base = dict(B=300, K=1, unbiased=True, importance_sampling=True, coef=COEF, kl_cutoff=None, grad_scale=1.0,
                clip_range_vf=None)
    cases.append(dict(base, kl_cutoff=1e-4))
    cases.append(dict(base, grad_scale=1.0 / 3.0))
    cases.append(dict(base, clip_range_vf=0.2))
    return cases


def loss_inputs(i: int, c: dict) -> dict:
    rng = np.random.default_rng(1000 + i)
    B, K = c["B"], c["K"]
    f = lambda a: np.asarray(a, np.float32)
    l = f(-np.abs(rng.standard_normal(B)) - 0.05)
    noise = rng.standard_normal(B) * 0.1
    k = len(noise[::5])  # |l - o| in [0.3, 0.7]: ratios outside [0.8, 1.2] on both sides
    noise[::5] = np.where(rng.random(k) < 0.5, -1.0, 1.0) * (0.3 + 0.4 * rng.random(k))
    o = f(l - f(noise))
    d = f(rng.uniform(-3.0, 3.0, B))
    d[::7] = 0.0
    t = f(l + d)
    t[::7] = l[::7]
    vs = (B,) if K == 1 else (B, K)
    v = f(rng.standard_normal(vs))
    vo = f(v + rng.standard_normal(vs) * 0.3)
    adv = f(rng.standard_normal(vs) * 2)
    return dict(new_logp=l, old_logp=o, teacher_logp=t, entropy=f(np.abs(rng.standard_normal(B)) * 0.5),
                new_values=v, old_values=vo, advantages=adv, returns=f(vo + adv))


def ppo_loss(mg, c: dict, x: dict, dt):
    """ppo.py:307-374 over given network outputs, with the reference's TeacherKLLoss."""
    from rl_algo_impls.loss.teacher_kl_loss import TeacherKLLoss

    T = lambda a: torch.from_numpy(a).to(dt)
    l = T(x["new_logp"]).requires_grad_(True)
    ent = T(x["entropy"]).requires_grad_(True)
    v = T(x["new_values"]).requires_grad_(True)
    o, vo, adv, ret = T(x["old_logp"]), T(x["old_values"]), T(x["advantages"]), T(x["returns"])
    adv = (adv - adv.mean(0)) / (adv.std(0) + 1e-8)
    if c["K"] > 1:
        adv = adv @ torch.tensor(MRW, dtype=torch.float32).to(dt)
    logratio = l - o
    ratio = torch.exp(logratio)
    clipped = torch.clamp(ratio, min=1 - 0.2, max=1 + 0.2)
    pi_loss = -torch.min(ratio * adv, clipped * adv).mean()
    vl = torch.nn.functional.mse_loss(v, ret, reduction="none")
    if c["clip_range_vf"] is not None:
        vc = c["clip_range_vf"]
        vl = torch.max(vl, torch.nn.functional.mse_loss(vo + torch.clamp(v - vo, -vc, vc), ret, reduction="none"))
    vl = vl.mean(0)
    ent_loss = -ent.mean()
    approx_kl = ((ratio - 1) - logratio).mean().item()
    pi_coef = 0 if (c["kl_cutoff"] is not None and approx_kl > c["kl_cutoff"]) else 1
    vf_coef = torch.tensor(0.5, dtype=torch.float32).to(dt)
    loss = pi_coef * pi_loss + 0.01 * ent_loss + (vf_coef * vl).sum()
    fn = TeacherKLLoss(None, unbiased=c["unbiased"])
    term = fn(l, {"teacher_logprobs": T(x["teacher_logp"])}, ratio if c["importance_sampling"] else None)
    loss = loss + c["coef"] * term
    if c["grad_scale"] != 1.0:
        loss = loss / round(1.0 / c["grad_scale"])
    loss.backward()
    return dict(d_logp=l.grad.double().numpy(), d_v=v.grad.double().numpy(), loss=loss.item(),
                teacher_kl_loss=term.item(), pi_loss=pi_loss.item(), approx_kl=approx_kl, pi_coef=pi_coef)


def make_policy(mg, case):
    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    act = gs.MultiDiscrete(np.array(case["nvec"])) if case["nvec"] is not None else gs.Discrete(case["n_act"])
    env = mg.StubVecEnv(N_ENVS, gs.Box(-np.inf, np.inf, (case["obs_dim"],), np.float32), act)
    torch.manual_seed(7)
    return ActorCritic(env, **case["policy"]), env


def inits(shapes, seed: int):
    """Student and teacher parameters: two draws of the pong_init recipe, each with N(0, 0.2) added so the
    two policies' action distributions are well apart (the recipe's actor output gain is 0.01)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in (seed + 1, seed + 2):
        p = pong_init(shapes, seed=s)
        out.append((p + 0.2 * rng.standard_normal(p.shape)).astype(np.float32))
    return out


def step_inputs(case: dict) -> dict:
    rng = np.random.default_rng(case["seed"])
    n = T_STEPS * N_ENVS
    groups = list(case["nvec"]) if case["nvec"] is not None else [case["n_act"]]
    obs = rng.standard_normal((n, case["obs_dim"])).astype(np.float32)
    mask, act = masks_and_actions(rng, n, groups, case["masked"])
    return dict(obs=obs, actions=act if case["nvec"] is not None else act[:, 0], masks=mask,
                d_logp=(rng.standard_normal(n) * 0.1).astype(np.float32),
                d_v=(rng.standard_normal(n) * 0.2).astype(np.float32),
                advantages=(rng.standard_normal(n) * 2).astype(np.float32),
                perms=np.stack([rng.permutation(n) for _ in range(EPOCHS)]).astype(np.int64))


def run_steps(mg, case, f64: bool, init, teacher_init, batch_f32=None):
    from rl_algo_impls.loss.teacher_kl_loss import TeacherKLLoss
    from rl_algo_impls.rollout.rollout import Batch, Rollout
    from rl_algo_impls.shared.callbacks.summary_wrapper import SummaryWrapper

    dt = torch.float64 if f64 else torch.float32
    T = lambda a: torch.from_numpy(a).to(dt)
    M = lambda m: None if m is None else torch.from_numpy(m)

    def policy_of(flat):
        p, env = make_policy(mg, case)
        if f64:
            p = p.double()
            p.network._feature_extractor.preprocess = lambda obs: obs.double()
        load_flat(p, flat)
        return p, env

    policy, env = policy_of(init)
    teacher, _ = policy_of(teacher_init)
    x = step_inputs(case)
    if batch_f32 is None:  # made once by the f32 policy, shared (as the same bits) with the f64 run
        with torch.no_grad():
            lp, _, v = policy(T(x["obs"]), torch.from_numpy(x["actions"]), action_masks=M(x["masks"]))
        values = (v + T(x["d_v"])).float().numpy()
        batch_f32 = dict(obs=x["obs"], actions=x["actions"], logprobs=(lp + T(x["d_logp"])).float().numpy(),
                         values=values, advantages=x["advantages"],
                         returns=(values + x["advantages"]).astype(np.float32), perms=x["perms"])
        if x["masks"] is not None:
            batch_f32["masks"] = x["masks"]
    b = batch_f32
    full = Batch(T(b["obs"]), T(b["logprobs"]), torch.from_numpy(b["actions"]), M(b.get("masks")), None,
                 T(b["values"]), T(b["advantages"]), T(b["returns"]))
    perms = iter(torch.from_numpy(b["perms"]))

    class PermRollout(Rollout):  # VecRollout's add_to_batch / minibatches over a given flat batch and permutations
        y_true = b["returns"]
        y_pred = b["values"]
        total_steps = len(full)

        def num_minibatches(self, batch_size):
            return -(-len(full) // batch_size)

        def add_to_batch(self, map_fn, batch_size):
            parts = {}
            for i in range(0, len(full), batch_size):
                for k, v in map_fn(full[torch.arange(i, i + batch_size)]).items():
                    parts.setdefault(k, []).append(v)
            full.additional.update({k: torch.cat(v) for k, v in parts.items()})

        def minibatches(self, batch_size, shuffle=True):
            idx = next(perms)
            for i in range(0, len(full), batch_size):
                yield full[idx[i:i + batch_size]]

    class Gen:
        vec_env = env

        def rollout(self, gamma, gae_lambda):
            return PermRollout()

    class Holder:
        latest_checkpoint = teacher

    algo = mg.PPO(policy, torch.device("cpu"), SummaryWrapper(mg.SummaryWriter()),
                  teacher_kl_loss_fn=TeacherKLLoss(Holder()), **case["kw"])
    rec = dict(params=[], norms=[], loss=[], teacher_kl_loss=[], batch=b)
    orig = algo.optimizer_step

    def optimizer_step():
        g = flat64([p.grad if p.grad is not None else torch.zeros_like(p) for p in policy.parameters()])
        rec["norms"].append(float(np.sqrt(np.sum(g * g))))
        out = orig()
        rec["params"].append(flat64(policy.parameters()))
        return out

    algo.optimizer_step = optimizer_step
    real = mg.ppo_mod.TrainStepStats

    def tss(*args):
        rec["loss"].append(float(args[0]))
        rec["teacher_kl_loss"].append(float(args[7]["teacher_kl_loss"]))
        return real(*args)

    mg.ppo_mod.TrainStepStats = tss
    try:
        algo.learn_epoch(0, len(full), Gen(), None)
    finally:
        mg.ppo_mod.TrainStepStats = real
    # all epochs' steps are recorded here; the reference's TrainStats keeps the last epoch's only
    rec["teacher_logprobs"] = full.additional["teacher_logprobs"].double().numpy()
    assert len(rec["loss"]) == len(rec["params"]) == EPOCHS * 3
    return rec, [tuple(p.shape) for p in policy.parameters()]


def main():
    import make_golden as mg  # imports the reference with its stubs

    up32 = lambda e: np.nextafter(np.asarray(e, np.float32), np.float32(np.inf))  # never round an error down
    arrays = {}
    cases = loss_cases()
    index = dict(torch=torch.__version__, numpy=np.__version__, loss_cases=cases, mrw=MRW, steps={},
                 T=T_STEPS, N=N_ENVS, batch=BATCH, epochs=EPOCHS, ent_coef=0.01, vf_coef=0.5, clip_range=0.2)
    for i, c in enumerate(cases):
        x = loss_inputs(i, c)
        r32, r64 = ppo_loss(mg, c, x, torch.float32), ppo_loss(mg, c, x, torch.float64)
        assert r32["pi_coef"] == r64["pi_coef"] == (0 if c["kl_cutoff"] is not None else 1)
        P = f"L{i}_"
        for k, v in x.items():
            arrays[P + k] = v
        for k in ("d_logp", "d_v", "loss", "teacher_kl_loss", "pi_loss", "approx_kl"):
            arrays[P + k] = np.asarray(r64[k], np.float64)
            arrays[P + k + "_f32"] = np.asarray(r32[k], np.float32)
            arrays[P + k + "_err"] = up32(np.abs(np.asarray(r32[k], np.float64) - np.asarray(r64[k])).max())
    print(f"{len(cases)} loss-level cases; worst |f32 - f64| d_logp "
          f"{max(float(arrays[f'L{i}_d_logp_err']) for i in range(len(cases))):.3e}")
    for name, case in STEP_CASES.items():
        shapes = [tuple(p.shape) for p in make_policy(mg, case)[0].parameters()]
        init, teacher_init = inits(shapes, case["seed"])
        rec, _ = run_steps(mg, case, False, init, teacher_init)
        rec64, _ = run_steps(mg, case, True, init, teacher_init, rec["batch"])
        cut = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
        pmax = lambda v: np.array([np.abs(v[cut[j]:cut[j + 1]]).max() for j in range(len(shapes))], np.float32)
        P = f"{name}_"
        arrays[P + "init"], arrays[P + "teacher_init"] = init, teacher_init
        for k, v in rec["batch"].items():
            arrays[P + k] = v
        arrays[P + "params"] = np.stack(rec64["params"])
        arrays[P + "params_f32"] = np.stack(rec["params"]).astype(np.float32)
        arrays[P + "params_err"] = up32(np.stack([pmax(a - b) for a, b in zip(rec["params"], rec64["params"])]))
        for k in ("loss", "teacher_kl_loss", "norms"):
            arrays[P + k] = np.array(rec64[k])
            arrays[P + k + "_f32"] = np.array(rec[k], np.float32)
            arrays[P + k + "_err"] = np.abs(np.array(rec[k]) - np.array(rec64[k]))
        arrays[P + "teacher_logprobs"] = rec64["teacher_logprobs"]
        arrays[P + "teacher_logprobs_f32"] = rec["teacher_logprobs"].astype(np.float32)
        arrays[P + "teacher_logprobs_err"] = up32(np.abs(rec["teacher_logprobs"] - rec64["teacher_logprobs"]).max())
        index["steps"][name] = dict(case, shapes=[list(s) for s in shapes])
        print(f"{name}: P={cut[-1]} loss {arrays[P + 'loss']} teacher_kl {arrays[P + 'teacher_kl_loss']} "
              f"err params {arrays[P + 'params_err'].max():.3e} loss {arrays[P + 'loss_err'].max():.3e} "
              f"norms {arrays[P + 'norms_err'].max():.3e}")
    arrays["index"] = np.array(json.dumps(index))
    out = HERE / "teacher_kl_steps.npz"
    np.savez_compressed(out, **arrays)
    print("wrote", out.name, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
