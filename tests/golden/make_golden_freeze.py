"""Golden vectors for PPO's freeze_policy_head / freeze_value_head / freeze_backbone, from the REFERENCE
ITSELF (run on the CPU): its PPO.learn_epoch (rl_algo_impls/ppo/ppo.py:280-285,412-413: policy.freeze(...)
around the update) called several times on ONE PPO object, so the optimizer's per-tensor state['step'] comes
apart across the calls as it does in a fine-tuning run.

Case `cat`: obs Box(4,), Discrete(2), hidden [8, 8], tanh (the policy of make_golden_teacher's `cat`);
T x N = 5 x 8 = 40 rows, batch 16 (minibatches 16 / 16 / 8), 2 epochs with fixed permutations: 6 optimizer
steps per update.  Three updates, each on a fresh seeded batch:

  (a) freeze_policy_head + freeze_backbone   only the critic steps (the Flatten backbone has no parameters)
  (b) nothing frozen                          the actor starts at step 1 while the critic is at step 7
  (c) freeze_value_head

Recorded per optimizer step: loss and the pre-clip gradient norm (over the tensors that have a gradient: what
clip_grad_norm_ returns); per update: all parameters; at the end of every update: the optimizer's state_dict
(per parameter `step`, `exp_avg`, `exp_avg_sq`; `has_state` marks the parameters that have an entry).

Case `impala`: the network of make_golden_impala.py (uint8 3x20x12, Categorical(15), cnn_flatten_dim 256;
P = 151,120), three fixed minibatches of 32 rows, 1 epoch: 3 optimizer steps per update.  Two updates, each
on fresh seeded minibatches: (a) freeze_backbone + freeze_policy_head, (b) nothing frozen (the critic head is
then at steps 4..6, everything else at 1..3).  Same per-step records.  To keep the file under the
repository's 1 MiB limit for a committed file, the large vectors are kept in reduced form: after (a) only
the critic head's tensors (the generator asserts every other tensor equals the initial value); after (b)
the float64 parameter vector rounded to float32 (`impala_params_u1`: a representation error of 2^-24 |ref|,
170 times below the 1e-5 |ref| term of the tests' bound) with the per-tensor `_err` taken from the unrounded
runs; of the final moments, per tensor the L2 norm in both precisions (as impala_steps.npz keeps them), and
the actor and critic heads' moments in full.

Everything is run in float32 and, from the same bits, in float64.  The float64 result is the record
(`<name>`), the float32 one is kept next to it (`<name>_f32`), and `<name>_err` is |f32 - f64| (per tensor
for parameters and moments: the maximum over the tensor's elements).

Asserted here: after each frozen update the frozen tensors equal their previous values exactly, in both
precisions; and in (b), re-running the update on a copy whose state['step'] are all forced equal moves some
actor parameter by more than 100 x its `_err` (the fixture tells per-tensor step counts from a single one).

    python tests/golden/make_golden_freeze.py            # writes freeze_steps.npz
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

from make_golden_multidiscrete import flat64, load_flat  # noqa: E402
from make_golden_teacher import BATCH, EPOCHS, N_ENVS, STEP_CASES, T_STEPS, inits, make_policy, step_inputs  # noqa: E402

CAT = dict(STEP_CASES["cat"], kw=dict(learning_rate=3e-4, batch_size=BATCH, n_epochs=EPOCHS, clip_range=0.2,
                                      ent_coef=0.01, vf_coef=0.5))
# (freeze_policy_head, freeze_value_head, freeze_backbone) per update
UPDATES = [dict(freeze_policy_head=True, freeze_value_head=False, freeze_backbone=True),
           dict(freeze_policy_head=False, freeze_value_head=False, freeze_backbone=False),
           dict(freeze_policy_head=False, freeze_value_head=True, freeze_backbone=False)]
STEPS_PER_UPDATE = EPOCHS * 3


def run_cat(mg, f64: bool, init, batches_f32=None, force_equal_steps_in=None):
    """The three updates; batches_f32: made by the float32 run, shared as the same bits.
    force_equal_steps_in: index of an update before which every state['step'] is set to the maximum one
    (the single-step-count optimizer this fixture must tell apart); the run stops after that update."""
    from rl_algo_impls.rollout.rollout import Batch, Rollout
    from rl_algo_impls.shared.callbacks.summary_wrapper import SummaryWrapper

    case = CAT
    dt = torch.float64 if f64 else torch.float32
    T = lambda a: torch.from_numpy(a).to(dt)
    policy, env = make_policy(mg, case)
    if f64:
        policy = policy.double()
        policy.network._feature_extractor.preprocess = lambda obs: obs.double()
    load_flat(policy, init)
    algo = mg.PPO(policy, torch.device("cpu"), SummaryWrapper(mg.SummaryWriter()), **case["kw"])
    params = list(policy.parameters())
    groups = dict(actor=[id(p) for p in policy.network._pi.parameters()],
                  critic=[id(p) for p in policy.network._v.parameters()],
                  backbone=[id(p) for p in policy.network._feature_extractor.parameters()])
    rec = dict(params=[], norms=[], loss=[], steps=[], has_state=[], exp_avg=[], exp_avg_sq=[], batches=[])
    orig = algo.optimizer_step

    def optimizer_step():
        norm = orig()
        rec["norms"].append(float(norm))
        return norm

    algo.optimizer_step = optimizer_step
    real = mg.ppo_mod.TrainStepStats

    def tss(*args):
        rec["loss"].append(float(args[0]))
        return real(*args)

    for u, flags in enumerate(UPDATES):
        x = step_inputs(dict(case, seed=case["seed"] + 10 * u))
        if batches_f32 is None:
            with torch.no_grad():
                lp, _, v = policy(T(x["obs"]), torch.from_numpy(x["actions"]))
            values = (v + T(x["d_v"])).float().numpy()
            b = dict(obs=x["obs"], actions=x["actions"], logprobs=(lp + T(x["d_logp"])).float().numpy(),
                     values=values, advantages=x["advantages"], returns=(values + x["advantages"]).astype(np.float32),
                     perms=x["perms"])
        else:
            b = batches_f32[u]
        rec["batches"].append(b)
        full = Batch(T(b["obs"]), T(b["logprobs"]), torch.from_numpy(b["actions"]), None, None, T(b["values"]),
                     T(b["advantages"]), T(b["returns"]))
        perms = iter(torch.from_numpy(b["perms"]))

        class PermRollout(Rollout):
            y_true = b["returns"]
            y_pred = b["values"]
            total_steps = len(full)

            def num_minibatches(self, batch_size):
                return -(-len(full) // batch_size)

            def add_to_batch(self, map_fn, batch_size):
                raise AssertionError("no teacher here")

            def minibatches(self, batch_size, shuffle=True):
                idx = next(perms)
                for i in range(0, len(full), batch_size):
                    yield full[idx[i:i + batch_size]]

        class Gen:
            vec_env = env

            def rollout(self, gamma, gae_lambda):
                return PermRollout()

        for k, v in flags.items():
            setattr(algo, k, v)
        if force_equal_steps_in == u:
            top = max(float(s["step"]) for s in algo.optimizer.state.values())
            for p in params:  # a tensor without state yet: zero moments at the shared count
                s = algo.optimizer.state[p]
                if len(s) == 0:
                    s["exp_avg"], s["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                s["step"] = torch.tensor(top)
        before = [p.detach().clone() for p in params]
        mg.ppo_mod.TrainStepStats = tss
        try:
            algo.learn_epoch(0, len(full), Gen(), None)
        finally:
            mg.ppo_mod.TrainStepStats = real
        assert all(p.requires_grad for p in params), "unfreeze() ran"
        frozen = set()
        for name, flag in (("actor", "freeze_policy_head"), ("critic", "freeze_value_head"),
                           ("backbone", "freeze_backbone")):
            if flags[flag]:
                frozen |= set(groups[name])
        for p, p0 in zip(params, before):
            if id(p) in frozen:
                assert torch.equal(p.detach(), p0), "a frozen tensor moved"
            else:
                assert not torch.equal(p.detach(), p0), "a trainable tensor stayed"
        rec["params"].append(flat64(params))
        st = [algo.optimizer.state.get(p) for p in params]
        rec["has_state"].append(np.array([s is not None and len(s) > 0 for s in st]))
        rec["steps"].append(np.array([float(s["step"]) if s else 0.0 for s in st]))
        zeros = lambda p: torch.zeros_like(p)
        rec["exp_avg"].append(flat64([s["exp_avg"] if s else zeros(p) for s, p in zip(st, params)]))
        rec["exp_avg_sq"].append(flat64([s["exp_avg_sq"] if s else zeros(p) for s, p in zip(st, params)]))
        if force_equal_steps_in == u:
            break
    return rec, [tuple(p.shape) for p in params], [[k for k, v in groups.items() if id(p) in v][0] for p in params]


IMPALA_KW = dict(learning_rate=5e-4, batch_size=32, clip_range=0.2, clip_range_vf=0.2, vf_coef=0.5, ent_coef=0.01)
IMPALA_UPDATES = [dict(freeze_policy_head=True, freeze_value_head=False, freeze_backbone=True),
                  dict(freeze_policy_head=False, freeze_value_head=False, freeze_backbone=False)]


def run_impala(mg, policy, f64: bool, batches_f32=None):
    """The two updates on one PPO object.  f64: `policy` is the double copy (the caller has patched the
    prescale); batches_f32: the float32 run's minibatches, reused as the same bits."""
    from rl_algo_impls.rollout.rollout import Batch
    from rl_algo_impls.shared.callbacks.summary_wrapper import SummaryWrapper

    from make_golden_impala import N_ACTIONS, OBS_SHAPE

    algo = mg.PPO(policy, torch.device("cpu"), SummaryWrapper(mg.SummaryWriter()), n_epochs=1, **IMPALA_KW)
    params = list(policy.parameters())
    net = policy.network
    group_of = []
    for p in params:
        group_of.append("actor" if any(p is q for q in net._pi.parameters()) else
                        "critic" if any(p is q for q in net._v.parameters()) else "backbone")
    rec = dict(params=[], norms=[], loss=[], steps=[], has_state=[], batches=[])
    orig = algo.optimizer_step

    def optimizer_step():
        norm = orig()
        rec["norms"].append(float(norm))
        return norm

    algo.optimizer_step = optimizer_step
    real = mg.ppo_mod.TrainStepStats

    def tss(*args):
        rec["loss"].append(float(args[0]))
        return real(*args)

    rng = np.random.default_rng(23)
    flag_of = dict(actor="freeze_policy_head", critic="freeze_value_head", backbone="freeze_backbone")
    for u, flags in enumerate(IMPALA_UPDATES):
        if batches_f32 is None:
            bs = [mg.make_batch(policy, 32, rng, OBS_SHAPE, discrete_n=N_ACTIONS, obs_u8=True) for _ in range(3)]
        else:
            bs = [Batch(b.obs, b.logprobs.double(), b.actions, None, None, b.values.double(), b.advantages.double(),
                        b.returns.double()) for b in batches_f32[u]]
        rec["batches"].append(bs)
        for k, v in flags.items():
            setattr(algo, k, v)
        before = [p.detach().clone() for p in params]
        mg.ppo_mod.TrainStepStats = tss
        try:
            r = mg.FixedRollout(bs)
            algo.learn_epoch(0, r.total_steps, mg.FixedGen(r), None)
        finally:
            mg.ppo_mod.TrainStepStats = real
        for p, p0, g in zip(params, before, group_of):
            assert torch.equal(p.detach(), p0) == flags[flag_of[g]], "frozen tensors stay, trainable ones move"
        rec["params"].append(flat64(params))
        st = [algo.optimizer.state.get(p) for p in params]
        rec["has_state"].append(np.array([bool(s) for s in st]))
        rec["steps"].append(np.array([float(s["step"]) if s else 0.0 for s in st]))
    rec["exp_avg"] = [s["exp_avg"].detach().double().numpy().reshape(-1) for s in st]
    rec["exp_avg_sq"] = [s["exp_avg_sq"].detach().double().numpy().reshape(-1) for s in st]
    return rec, group_of


def impala_arrays(mg, up32) -> tuple:
    import copy

    import gymnasium.spaces as gs  # (stub)

    from rl_algo_impls.shared.encoder import cnn as cnn_mod
    from rl_algo_impls.shared.policy.actor_critic import ActorCritic

    from make_golden_impala import N_ACTIONS, OBS_SHAPE, POLICY_KW
    from make_golden_pong import INIT_SEED, pong_init

    env = mg.StubVecEnv(1, gs.Box(0, 255, OBS_SHAPE, np.uint8), gs.Discrete(N_ACTIONS), kind="pong")
    torch.manual_seed(7)
    policy = ActorCritic(env, **POLICY_KW)
    shapes = [tuple(p.shape) for p in policy.parameters()]
    init = pong_init(shapes)
    load_flat(policy, init)
    policy64 = copy.deepcopy(policy).double()
    r32, group_of = run_impala(mg, policy, False)
    real_pre = cnn_mod.CnnEncoder.preprocess

    def preprocess64(self, obs):
        if len(obs.shape) == 3:
            obs = obs.unsqueeze(0)
        return obs.double() / self.range_size

    cnn_mod.CnnEncoder.preprocess = preprocess64
    try:
        r64, _ = run_impala(mg, policy64, True, r32["batches"])
    finally:
        cnn_mod.CnnEncoder.preprocess = real_pre
    sizes = [int(np.prod(s)) for s in shapes]
    cut = np.cumsum([0] + sizes)
    pmax = lambda v: np.array([np.abs(v[cut[j]:cut[j + 1]]).max() for j in range(len(shapes))], np.float32)
    P, a = "impala_", {}
    for u, bs in enumerate(r32["batches"]):
        for i, b in enumerate(bs):
            for f in ("obs", "logprobs", "actions", "values", "advantages", "returns"):
                a[f"{P}u{u}_b{i}_{f}"] = getattr(b, f).numpy()
    for k in ("loss", "norms"):
        a[P + k] = np.array(r64[k])
        a[P + k + "_f32"] = np.array(r32[k], np.float32)
        a[P + k + "_err"] = np.abs(np.array(r32[k]) - np.array(r64[k]))
    for k in ("steps", "has_state"):
        assert all(np.array_equal(x, y) for x, y in zip(r32[k], r64[k]))
        a[P + k] = np.stack(r32[k])
    a[P + "params_err"] = up32(np.stack([pmax(x - y) for x, y in zip(r32["params"], r64["params"])]))
    critic = np.concatenate([np.arange(cut[j], cut[j + 1]) for j, g in enumerate(group_of) if g == "critic"])
    rest = np.setdiff1d(np.arange(cut[-1]), critic)
    assert np.array_equal(r32["params"][0][rest], init[rest].astype(np.float64))
    assert np.array_equal(r64["params"][0][rest], init[rest].astype(np.float64))
    a[P + "params_u0_critic"] = r64["params"][0][critic]
    a[P + "params_u0_critic_f32"] = r32["params"][0][critic].astype(np.float32)
    a[P + "params_u1"] = r64["params"][1].astype(np.float32)  # (rounded: see the module docstring)
    l2 = lambda ts: np.array([np.sqrt(np.sum(np.square(t))) for t in ts])
    for k in ("exp_avg", "exp_avg_sq"):
        a[P + k + "_norms"] = l2(r64[k])
        a[P + k + "_norms_f32"] = l2(r32[k]).astype(np.float32)
        a[P + k + "_norms_err"] = np.abs(l2(r32[k]) - l2(r64[k]))
        heads = [j for j, g in enumerate(group_of) if g != "backbone"]
        a[P + k + "_heads"] = np.concatenate([r64[k][j] for j in heads])
        a[P + k + "_heads_f32"] = np.concatenate([r32[k][j] for j in heads]).astype(np.float32)
        a[P + k + "_heads_err"] = up32(np.array([np.abs(r32[k][j] - r64[k][j]).max() for j in heads]))
    meta = dict(kw=IMPALA_KW, n=3, B=32, shapes=[list(s) for s in shapes], groups=group_of, init_seed=INIT_SEED,
                policy=POLICY_KW, obs_shape=list(OBS_SHAPE), n_actions=N_ACTIONS, updates=IMPALA_UPDATES,
                steps_per_update=3)
    print(f"impala: P={cut[-1]} steps after (a) {sorted(set(a[P + 'steps'][0]))} after (b) {sorted(set(a[P + 'steps'][1]))} "
          f"norms {a[P + 'norms']} err norms {a[P + 'norms_err']} loss {a[P + 'loss_err']} "
          f"params err max {a[P + 'params_err'].max():.3e}")
    return a, meta


def main():
    import make_golden as mg  # imports the reference with its stubs

    up32 = lambda e: np.nextafter(np.asarray(e, np.float32), np.float32(np.inf))  # never round an error down
    shapes = [tuple(p.shape) for p in make_policy(mg, CAT)[0].parameters()]
    init = inits(shapes, CAT["seed"])[0]
    r32, _, group_of = run_cat(mg, False, init)
    r64, _, _ = run_cat(mg, True, init, r32["batches"])
    cut = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    pmax = lambda v: np.array([np.abs(v[cut[j]:cut[j + 1]]).max() for j in range(len(shapes))], np.float32)
    arrays = {"cat_init": init}
    P = "cat_"
    for u, b in enumerate(r32["batches"]):
        for k, v in b.items():
            arrays[f"{P}u{u}_{k}"] = v
    for k in ("params", "exp_avg", "exp_avg_sq"):
        arrays[P + k] = np.stack(r64[k])
        arrays[P + k + "_f32"] = np.stack(r32[k]).astype(np.float32)
        arrays[P + k + "_err"] = up32(np.stack([pmax(a - b) for a, b in zip(r32[k], r64[k])]))
    for k in ("loss", "norms"):
        arrays[P + k] = np.array(r64[k])
        arrays[P + k + "_f32"] = np.array(r32[k], np.float32)
        arrays[P + k + "_err"] = np.abs(np.array(r32[k]) - np.array(r64[k]))
    assert len(r32["loss"]) == len(r32["norms"]) == STEPS_PER_UPDATE * len(UPDATES)
    for k in ("steps", "has_state"):
        assert all(np.array_equal(a, b) for a, b in zip(r32[k], r64[k]))
        arrays[P + k] = np.stack(r32[k])
    # the fixture tells per-tensor step counts from one shared count: (b) re-run with every step forced equal
    alt, _, _ = run_cat(mg, True, init, r32["batches"], force_equal_steps_in=1)
    d = np.abs(alt["params"][1] - r64["params"][1])
    actor = np.concatenate([np.full(cut[j + 1] - cut[j], group_of[j] == "actor") for j in range(len(shapes))])
    err = np.concatenate([np.full(cut[j + 1] - cut[j], arrays[P + "params_err"][1][j], np.float64)
                          for j in range(len(shapes))])
    ratio = float((d[actor] / err[actor]).max())
    assert ratio > 100, ratio
    index = dict(torch=torch.__version__, numpy=np.__version__, T=T_STEPS, N=N_ENVS, batch=BATCH, epochs=EPOCHS,
                 steps_per_update=STEPS_PER_UPDATE, updates=UPDATES,
                 cat=dict(CAT, shapes=[list(s) for s in shapes], groups=group_of, single_step_ratio=ratio))
    ia, index["impala"] = impala_arrays(mg, up32)
    arrays.update(ia)
    arrays["index"] = np.array(json.dumps(index))
    out = HERE / "freeze_steps.npz"
    np.savez_compressed(out, **arrays)
    print(f"cat: P={cut[-1]} steps {arrays[P + 'steps'].tolist()} norms {arrays[P + 'norms']}")
    print(f"  err params {arrays[P + 'params_err'].max():.3e} loss {arrays[P + 'loss_err'].max():.3e} "
          f"norms {arrays[P + 'norms_err'].max():.3e}; forcing one step count moves an actor weight by "
          f"{ratio:.0f} x its err")
    print("wrote", out.name, out.stat().st_size, "bytes")
    assert out.stat().st_size < 2 ** 20


if __name__ == "__main__":
    main()
