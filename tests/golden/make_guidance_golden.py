#!/usr/bin/env python3
"""Golden vectors for the classical guidance baselines and the per-episode evaluator of the reference's paper
benchmark (rl_system/scripts/paper_benchmark_suite.py): the reference's own `PurePursuit` (:171),
`ProportionalNavigation` (:92), `AugmentedPN` (:135) and `PolicyEvaluator.evaluate_classical_policy` (:212-298) with
`_compute_aggregate_metrics` (:366-398), run unchanged over a few short episodes of three scenarios (one a volley).
Runs ONLY where the reference exists; writes tests/golden/guidance/*.npz (plain data).

Recorded per case (one law, one scenario, one seed): what every `get_action` call saw and returned, every environment
step's outputs (obs, reward and its Python type, terminated / truncated, the info positions, `intercepted`), the
reset observations, the reference's `episode_data` list and its aggregate dict.  `synthetic.npz` drives `get_action`
alone over hand-made observations that sit on the branch boundaries (lock quality one ulp around 0.3 / 0.5, relative
position norms around 1e-6, LOS rates that saturate the clip, an APN first call followed by coast calls).

The reference's radar and wind models draw from entropy-seeded generators (`np.random.default_rng()`, core.py:270,
physics_models.py:298), so `np.random.seed(seed)` alone does not make its evaluator repeatable; while a case runs, an
unseeded `default_rng()` call is given the seed (case seed, call index).  Nothing else about the reference changes.

`make_guidance_golden.py --check` regenerates every fixture into a scratch directory and compares them bit for bit.
"""
import copy
import importlib.util
import os
import sys
import tempfile

sys.dont_write_bytecode = True
import numpy as np

REF = "/root/reference/rl_system"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "guidance")

# (fixture, scenario, physics, overrides, episodes, seed).  max_steps is cut short so that the fixtures stay small.
# 'long': episodes that end before max_steps (the pursuit laws do not reach the missile: closest approach > 2 km);
# 'kill_radius': the same start with the config's proximity_kill_radius at 3000 m, which the closest approaches fall on both
# sides of (success decided by the distance); 'close_weak_radar': the missile spawns 1 km away and flies at the interceptor,
# so that `intercepted` fires (success with a closest approach above the default radius of 50), and the onboard radar's
# quality is 0.45, so that a detection scales the track quality below 0.5 and a miss leaves it above: lock losses and
# recoveries on most steps (core.py:891-896).
_CLOSE = {"missile_spawn.position": [[600, 600, 600], [700, 700, 700]], "missile_spawn.velocity": [[-250, -250, -120], [-300, -300, -150]]}
CASES = [
    ("medium_base", "medium", "base", {"max_steps": 60}, 3, 11),
    ("hard_v2", "hard", "v2", {"max_steps": 60}, 3, 12),
    ("volley3_medium_config", "medium", "config", {"max_steps": 60, "volley_mode": True, "volley_size": 3}, 3, 13),
    ("medium_base_long", "medium", "base", {"max_steps": 700}, 2, 14),
    ("medium_base_kill_radius", "medium", "base", {"max_steps": 500, "proximity_kill_radius": 3000.0}, 3, 15),
    ("medium_base_close_weak_radar", "medium", "base", dict(_CLOSE, max_steps=300, radar={"radar_quality": 0.45}), 3, 16),
]
FIELDS = ("episode_id", "min_distance", "final_distance", "steps", "total_reward", "fuel_used", "lock_losses",
          "lock_recoveries", "success")


def _gen_module():
    spec = importlib.util.spec_from_file_location("_make_golden", os.path.join(HERE, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _laws(suite):
    return [suite.PurePursuit(), suite.ProportionalNavigation(N=3.0, use_true_state=True),
            suite.ProportionalNavigation(N=4.0, use_true_state=False), suite.AugmentedPN(N=4.0, K_acc=0.5)]


def _law_params(p):
    kind = {"PurePursuit": 1, "ProportionalNavigation": 2, "AugmentedPN": 3}[type(p).__name__]
    return dict(law_kind=np.int64(kind), law_name=np.array(p.name), law_N=np.float64(getattr(p, "N", 0.0)),
                law_K=np.float64(getattr(p, "K_acc", 0.0)), law_true=np.int64(bool(getattr(p, "use_true_state", False))))


def run_case(suite, environment, fname, env_cfg, policy, n_episodes, seed, out):
    rec = {k: [] for k in ("obs_in", "action", "obs", "reward", "terminated", "truncated", "int_pos", "mis_pos",
                           "intercepted", "reset_obs", "ep_start")}
    rtypes = []
    orig_step, orig_reset, orig_get = environment.InterceptEnvironment.step, environment.InterceptEnvironment.reset, policy.get_action

    def step(self, action):
        o, r, te, tr, info = orig_step(self, action)
        rec["obs"].append(np.array(o, np.float32))
        rec["reward"].append(np.float64(r))
        rtypes.append(type(r).__name__)
        rec["terminated"].append(bool(te))
        rec["truncated"].append(bool(tr))
        rec["int_pos"].append(np.array(info["interceptor_pos"]))
        rec["mis_pos"].append(np.array(info["missile_pos"]))
        rec["intercepted"].append(bool(info.get("intercepted", False)))
        return o, r, te, tr, info

    def reset(self, *a, **k):
        o, info = orig_reset(self, *a, **k)
        rec["reset_obs"].append(np.array(o, np.float32))
        rec["ep_start"].append(len(rec["obs"]))
        return o, info

    def get_action(obs, info=None):
        a = orig_get(obs, info)
        rec["obs_in"].append(np.array(obs, np.float32))
        rec["action"].append(np.array(a))
        return a

    orig_rng, calls = np.random.default_rng, []

    def default_rng(seed=None):
        if seed is None:
            calls.append(None)
            seed = [int(env_cfg.get("max_steps", 0)), seed_, len(calls)]
        return orig_rng(seed)

    seed_ = int(seed)
    environment.InterceptEnvironment.step, environment.InterceptEnvironment.reset = step, reset
    policy.get_action = get_action
    np.random.default_rng = default_rng
    try:
        ev = object.__new__(suite.PolicyEvaluator)
        ev.config = {"environment": copy.deepcopy(env_cfg)}
        res = ev.evaluate_classical_policy(policy, n_episodes, seed)
    finally:
        np.random.default_rng = orig_rng
        environment.InterceptEnvironment.step, environment.InterceptEnvironment.reset = orig_step, orig_reset
        del policy.get_action
    # the reward is np.float32, except the terminal bonuses / penalties (environment.py:1148-1287), which are Python floats
    assert set(rtypes) <= {"float32", "float"}, set(rtypes)
    eps = res["episodes"]
    ep = {}
    for f in FIELDS:
        vals = [e[f] for e in eps]
        ep["ep_" + f] = np.array([np.nan if v is None else v for v in vals])
        ep["ep_type_" + f] = np.array(type(vals[0]).__name__)
    agg_keys = sorted(k for k in res if k not in ("policy_name", "n_episodes", "seed", "episodes"))
    agg = np.array([np.nan if res[k] is None else float(res[k]) for k in agg_keys], np.float64)
    assert rec["int_pos"][0].dtype == np.float32 and rec["action"][0].dtype == np.float32
    np.savez_compressed(os.path.join(out, fname + ".npz"),
                        obs_in=np.stack(rec["obs_in"]), action=np.stack(rec["action"]), obs=np.stack(rec["obs"]),
                        reward=np.array(rec["reward"], np.float64), reward_pyfloat=np.array([t == "float" for t in rtypes]),
                        terminated=np.array(rec["terminated"]), truncated=np.array(rec["truncated"]),
                        int_pos=np.stack(rec["int_pos"]), mis_pos=np.stack(rec["mis_pos"]), intercepted=np.array(rec["intercepted"]),
                        reset_obs=np.stack(rec["reset_obs"]), ep_start=np.array(rec["ep_start"], np.int64),
                        kill_radius=np.float64(env_cfg.get("proximity_kill_radius", 50)), seed=np.int64(seed),
                        n_episodes=np.int64(n_episodes), policy_name=np.array(res["policy_name"]),
                        agg_keys=np.array(agg_keys), agg_values=agg, **ep, **_law_params(policy))
    print(f"{fname:48s} steps={len(rec['obs']):5d} python-float rewards={rtypes.count('float')} success={[bool(e['success']) for e in eps]} "
          f"steps/ep={[e['steps'] for e in eps]}")


def synthetic_obs(rng):
    """Observations on the laws' branch boundaries; every other entry random within the observation box."""
    rows = []
    f = np.float32

    def row(lock=0.8, rel=None, los=None):
        o = rng.uniform(-2, 1, 26).astype(np.float32)
        o[14] = lock
        if rel is not None:
            o[0:3] = rel
        if los is not None:
            o[2:4] = los
        return o

    # lock quality one ulp around the coast threshold (0.3) and the lock threshold (0.5)
    for c in (f(0.3), f(0.5)):
        for v in (np.nextafter(c, f(0)), c, np.nextafter(c, f(1))):
            rows.append(row(lock=v))
    # relative position norms around 1e-6 (the pursuit law's degenerate-bearing branch)
    for s in (2e-7, 5.7e-7, 5.773502e-7, 5.7735027e-7, 5.78e-7, 1e-6, 3e-6):
        rows.append(row(rel=np.full(3, s, np.float32)))
    for s in (9.99e-7, 1e-6, 1.0001e-6):
        rows.append(row(rel=np.array([s, 0, 0], np.float32)))
    rows.append(row(rel=np.zeros(3, np.float32)))
    # LOS rates that saturate the clip, both signs, and just inside it
    for los in ((0.9, -0.95), (-1.5, 1.7), (0.25, -0.25), (0.2500001, 0.6666667), (-0.3333334, 0.5), (1.0, -2.0)):
        rows.append(row(los=np.array(los, np.float32)))
    # coast calls between lock calls (APN's previous rate must stay where the last lock call left it)
    for k in range(12):
        rows.append(row(lock=f(0.1) if k % 3 else f(0.9), los=rng.uniform(-0.6, 0.6, 2).astype(np.float32)))
    for k in range(40):
        rows.append(row(lock=rng.uniform(0.0, 1.0), rel=(rng.standard_normal(3) * 10.0 ** rng.uniform(-8, 0)).astype(np.float32)))
    return np.stack(rows)


def synthetic(suite, out):
    rng = np.random.default_rng(7)
    # the APN sequence begins with two coast calls, then its first lock call (float64 previous rate), then coast calls
    head = np.stack([np.r_[rng.uniform(-2, 1, 14), 0.1, rng.uniform(-2, 1, 11)] for _ in range(2)] +
                    [np.r_[rng.uniform(-2, 1, 2), 0.31, -0.47, rng.uniform(-2, 1, 10), 0.95, rng.uniform(-2, 1, 11)]] +
                    [np.r_[rng.uniform(-2, 1, 14), 0.2, rng.uniform(-2, 1, 11)] for _ in range(3)]).astype(np.float32)
    obs = np.concatenate([head, synthetic_obs(rng)])
    laws = _laws(suite) + [suite.ProportionalNavigation(N=5.0, use_true_state=False), suite.AugmentedPN(N=3.0, K_acc=1.25)]
    acts, params = [], []
    for p in laws:
        acts.append(np.stack([p.get_action(o.copy(), {}) for o in obs]))
        params.append(_law_params(p))
    np.savez_compressed(os.path.join(out, "synthetic.npz"), obs_in=obs, actions=np.stack(acts),
                        **{k: np.array([pp[k] for pp in params]) for k in params[0]})
    print(f"synthetic: {len(obs)} observations x {len(laws)} laws")


def generate(out):
    mg = _gen_module()
    mg._install_gym_shim()
    sys.modules["gymnasium"].Env.close = lambda self: None      # gym.Env.close(): the evaluator calls it at the end (:293)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    import environment
    import paper_benchmark_suite as suite
    os.makedirs(out, exist_ok=True)
    for fname, scen, phys, over, n_ep, seed in CASES:
        cfg = mg.scenario_config(scen, phys, over)
        for p in _laws(suite):
            run_case(suite, environment, f"{fname}_{p.name}", cfg, p, n_ep, seed, out)
    synthetic(suite, out)


def _npz_equal(a, b):
    x, y = np.load(a), np.load(b)
    if sorted(x.files) != sorted(y.files):
        return f"keys {sorted(set(x.files) ^ set(y.files))}"
    for k in x.files:
        u, v = x[k], y[k]
        if u.dtype != v.dtype or u.shape != v.shape or u.tobytes() != v.tobytes():
            return f"array {k}"
    return None


def check():
    bad, n = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        generate(tmp)
        have = sorted(f for f in os.listdir(OUT) if f.endswith(".npz"))
        made = sorted(f for f in os.listdir(tmp) if f.endswith(".npz"))
        for f in sorted(set(have) | set(made)):
            n += 1
            if f not in have or f not in made:
                bad.append((f, "only " + ("committed" if f in have else "regenerated")))
            elif (why := _npz_equal(os.path.join(OUT, f), os.path.join(tmp, f))):
                bad.append((f, why))
    for f, why in bad:
        print("DIFFERS", f, why)
    print(f"check: {n - len(bad)} of {n} fixtures regenerate bit-identically")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        sys.exit(check())
    if os.path.isdir(OUT):
        for f in os.listdir(OUT):
            if f.endswith(".npz"):
                os.remove(os.path.join(OUT, f))
    generate(OUT)
