#!/usr/bin/env python3
"""Guided-evaluation rate on one MI355X: the closed loop of hlynr_intercept_amd/evaluation.py
(`hlx_eval_run`: step launch + evaluation launch per step, issued from C) at 65 536 environments, medium scenario, base
physics, PN_N4.0_radar -- host clock around a run that ends in a synchronise -- next to the same loop driven from Python
(`step_torch`, the law as torch ops, the bookkeeping as torch ops) and to the step alone (`hlx_rollout`).

  python tools/time_guidance.py [--envs 65536] [--steps 500] [--out FILE.json]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_guidance.py --kernels-only     (the launches alone, for the trace)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def python_loop(env, steps, torch):
    """step_torch + PN (N=4, radar) as torch ops + per-episode bookkeeping as torch ops: what the issue's 'shortest way
    through the existing API' costs.  Keeps the same accumulators as the kernel (no host round trip per step)."""
    n = env.num_envs
    obs = env.reset_torch()
    fuel0, was = obs[:, 12].clone(), obs[:, 14] > 0.5
    nsteps = torch.zeros(n, dtype=torch.int32, device=obs.device)
    ret = torch.zeros(n, device=obs.device)
    mind = torch.full((n,), float("inf"), device=obs.device)
    lastd = torch.zeros(n, device=obs.device)
    loss = torch.zeros(n, dtype=torch.int32, device=obs.device)
    rec = torch.zeros(n, dtype=torch.int32, device=obs.device)
    fuel_used = torch.zeros(n, device=obs.device)
    coast = torch.tensor([0.3, 0, 0, 0, 0, 0], device=obs.device)
    a = torch.zeros((n, 6), device=obs.device)
    a[:, 0] = 1.0
    for _ in range(steps):
        act = a.clone()
        act[:, 1:3] = (4.0 * (obs[:, 2:4] * 0.5)).clamp(-1.0, 1.0)
        act = torch.where((obs[:, 14] < 0.3)[:, None], coast, act)
        obs, r, te, tr, info = env.step_torch(act)
        done = (te | tr).bool()
        nsteps += 1
        ret += r
        d = (info["interceptor_pos"] - info["missile_pos"]).norm(dim=0)
        mind = torch.minimum(mind, d)
        lastd = d
        last = torch.where(done[:, None], env.terminal_obs, obs)
        locked = last[:, 14] > 0.5
        loss += (was & ~locked).int()
        rec += (~was & locked).int()
        fuel_used = torch.where(done, fuel0 - last[:, 12], fuel_used)
        was = torch.where(done, obs[:, 14] > 0.5, locked)
        fuel0 = torch.where(done, obs[:, 12], fuel0)
        for t_ in (nsteps, loss, rec):
            t_.masked_fill_(done, 0)
        ret.masked_fill_(done, 0.0)
        mind.masked_fill_(done, float("inf"))
    return lastd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    import torch

    from hlynr_intercept_amd import evaluation as E
    from hlynr_intercept_amd.scenarios import scenario_config
    from hlynr_intercept_amd.vec_env import HlynrVecEnv

    n, K = a.envs, a.steps
    cfg = scenario_config("medium", "base")
    env = HlynrVecEnv(config=cfg, num_envs=n, seed=1)
    ev = E.GuidanceEvaluator(n, E.ProportionalNavigation(4.0, False), 1, 50.0)
    out = {"envs": n, "steps": K, "scenario": "medium/base", "law": "PN_N4.0_radar", "kernel_baked": env.kernel_baked}
    ev.run(env, 50, 50)                                     # warm-up: code objects loaded, first launches paid
    torch.cuda.synchronize()
    if a.kernels_only:
        ev.run(env, K, K)
        torch.cuda.synchronize()
        print(json.dumps(out))
        return
    reps = []
    for _ in range(3):
        t0 = time.perf_counter()
        steps = ev.run(env, K, K)                           # one counter read at the end: it synchronises
        reps.append((time.perf_counter() - t0, steps))
    best = min(s / steps for s, steps in reps)
    out["guided"] = {"us_per_step": [s / st * 1e6 for s, st in reps], "best_us_per_step": best * 1e6, "env_steps_per_s": n / best}
    # the step alone, same form of launch (one per step from C), no evaluation kernel
    tape = torch.zeros((K, n, 6), device="cuda")
    env.reset_torch()
    env.rollout_torch(tape[:50])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env.rollout_torch(tape)
    torch.cuda.synchronize()
    st = (time.perf_counter() - t0) / K
    out["step_only_rollout"] = {"us_per_step": st * 1e6, "env_steps_per_s": n / st}
    # the Python-driven loop
    Kp = max(50, K // 2)
    python_loop(env, 20, torch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    python_loop(env, Kp, torch)
    torch.cuda.synchronize()
    pt = (time.perf_counter() - t0) / Kp
    out["python_loop"] = {"steps": Kp, "us_per_step": pt * 1e6, "env_steps_per_s": n / pt}
    out["speedup_vs_python_loop"] = pt / best
    ev.close()
    env.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
