"""Closed-loop evaluation on the device: the reference's paper benchmark (rl_system/scripts/paper_benchmark_suite.py) for N
environments at once.

* `PurePursuit`, `ProportionalNavigation`, `AugmentedPN` -- the three classical guidance laws (:92-195) with the reference's
  constructor arguments and `.name`.  They are specifications for the kernel (hlynr_intercept_amd/csrc/hlx_eval.inc), not
  numpy code: the law runs on the GPU behind every step launch, with no host involvement per step.
* `evaluate_classical_policy` -- `PolicyEvaluator.evaluate_classical_policy` (:212-298): per-episode records accumulated on
  the device, the reference's result dict back.
* `evaluate_policy` -- the same metrics for any `obs [N, 26] -> action [N, 6]` torch callable (e.g. a deterministic PPO
  forward); the step runs through `HlynrVecEnv.step_torch`, the bookkeeping in the same kernel without a law.
* `aggregate_metrics` -- `_compute_aggregate_metrics` (:366-398), host code.

Where the batch reads the reference's single sequence differently ("Evaluating guidance laws"):
* seeds give statistically equivalent runs, not the reference's trajectories: the environments draw from Philox streams
  keyed by (seed, environment, step), not from `np.random`;
* each environment carries its own AugmentedPN previous LOS rate: zero (float64, as the reference's `np.zeros(2)`) at the
  start of an evaluation, then carried across that environment's episodes, as the reference carries it across all of its;
* the episodes kept are the first `n_episodes` in (episode index, environment) order -- every environment's first episode,
  then every environment's second, ... -- so that short episodes, which finish first, are not favoured;
* the environment is a fresh one: the curriculum stays at step 0.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from . import _lib

RECORD_FIELDS = ("min_distance", "final_distance", "steps", "total_reward", "fuel_used", "lock_losses", "lock_recoveries", "success")
_RECORD_DTYPES = (np.float32, np.float32, np.int32, np.float32, np.float32, np.int32, np.int32, np.uint8)
# at most this many episodes come back as a list of dicts as well as arrays
EPISODE_DICTS_MAX = 10000


class PurePursuit:
    """Fly at the target bearing (paper_benchmark_suite.py:171-195)."""
    law = _lib.LAW_PURSUIT

    def __init__(self):
        self.name = "PurePursuit"


class ProportionalNavigation:
    """Proportional navigation (paper_benchmark_suite.py:92-132).  use_true_state: the reference looks for true LOS rates in
    `info`, which the environment never provides, and falls back to obs[2], obs[3] WITHOUT the radar variant's x 0.5."""
    law = _lib.LAW_PN

    def __init__(self, N: float = 3.0, use_true_state: bool = True):
        self.N = N
        self.use_true_state = use_true_state
        self.name = f"PN_N{N}" + ("_true" if use_true_state else "_radar")


class AugmentedPN:
    """Augmented proportional navigation (paper_benchmark_suite.py:135-168)."""
    law = _lib.LAW_APN

    def __init__(self, N: float = 4.0, K_acc: float = 0.5):
        self.N = N
        self.K_acc = K_acc
        self.name = f"AugPN_N{N}_K{K_acc}"


class GuidanceEvaluator:
    """The device evaluator (include/hlx_eval.h) for `n_envs` environments: `policy` one of the law classes above, or None for
    metrics only; `episodes_per_env` records kept per environment."""

    def __init__(self, n_envs: int, policy=None, episodes_per_env: int = 1, kill_radius: float = 50.0, device: int = 0):
        if policy is not None and not hasattr(policy, "law"):
            raise TypeError(f"{type(policy).__name__} is not one of PurePursuit, ProportionalNavigation, AugmentedPN")
        self._lib = _lib.load()
        self.n, self.E, self.device = int(n_envs), int(episodes_per_env), int(device)
        self.law = _lib.LAW_NONE if policy is None else policy.law
        cfg = _lib.HlxEvalConfig(n_envs=self.n, device=self.device, law=self.law,
                                 use_true_state=int(bool(getattr(policy, "use_true_state", False))), episodes_per_env=self.E,
                                 N=float(getattr(policy, "N", 0.0)), K_acc=float(getattr(policy, "K_acc", 0.0)),
                                 kill_radius=float(kill_radius))
        self._h = C.c_void_p()
        _lib.check(self._lib.hlx_eval_create(C.byref(cfg), C.byref(self._h)))

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    @staticmethod
    def _stream(device):
        import torch
        return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def begin(self, obs, actions=None):
        """obs [N, 26] device tensor of reset observations; actions [N, 6] receives the first action (law only)."""
        _lib.check(self._lib.hlx_eval_begin(self._h, obs.data_ptr(), self._ptr(actions), self._stream(self.device)))

    def observe(self, obs, reward, terminated, truncated, terminal_obs, packed=None, interceptor_pos=None, missile_pos=None,
                flags=None, actions=None):
        """One auto-resetting step's outputs (device tensors): the packed info words [3, N, 4], or the planes interceptor_pos /
        missile_pos [3, N] and flags [N]."""
        info = _lib.HlxInfoSoa(packed=self._ptr(packed), interceptor_pos=self._ptr(interceptor_pos),
                               missile_pos=self._ptr(missile_pos), flags=self._ptr(flags))
        _lib.check(self._lib.hlx_eval_observe(self._h, obs.data_ptr(), reward.data_ptr(), terminated.data_ptr(), truncated.data_ptr(),
                                              terminal_obs.data_ptr(), C.byref(info), self._ptr(actions), self._stream(self.device)))

    def run(self, env, max_steps: int, check_every: int = 64, action_tape=None) -> int:
        """Reset `env` (an HlynrVecEnv) and run the closed loop from C; returns the number of steps issued.  action_tape:
        optional device tensor [max_steps, N, 6] that receives every step's action."""
        steps = C.c_int64(0)
        _lib.check(self._lib.hlx_eval_run(self._h, env._h, int(max_steps), int(check_every), self._ptr(action_tape), C.byref(steps),
                                          self._stream(self.device)))
        return int(steps.value)

    def done_count(self) -> int:
        """Environments holding all their records (synchronises the current stream)."""
        out = C.c_int32(0)
        _lib.check(self._lib.hlx_eval_done_count(self._h, C.byref(out), self._stream(self.device)))
        return int(out.value)

    def records(self) -> Dict[str, np.ndarray]:
        """The record planes [E, N] (RECORD_FIELDS; success as bool) and 'episodes' [N], episodes finished per environment."""
        out = {f: np.zeros((self.E, self.n), dt) for f, dt in zip(RECORD_FIELDS, _RECORD_DTYPES)}
        out["episodes"] = np.zeros(self.n, np.int32)
        _lib.check(self._lib.hlx_eval_records(self._h, *(out[f].ctypes.data for f in RECORD_FIELDS), out["episodes"].ctypes.data,
                                              self._stream(self.device)))
        out["success"] = out["success"].astype(bool)
        return out

    def close(self):
        if self._h:
            self._lib.hlx_eval_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def select_episodes(records: Dict[str, np.ndarray], n_episodes: int) -> Dict[str, np.ndarray]:
    """The first n_episodes records in (episode index, environment) order, as 1-D arrays."""
    return {f: np.ascontiguousarray(records[f]).reshape(-1)[:n_episodes] for f in RECORD_FIELDS}


def episode_dicts(arrays: Dict[str, np.ndarray]) -> List[Dict[str, Any]]:
    """The reference's `episode_data` dicts (:240-250) from record arrays: float fields as np.float32, counts as int,
    min_distance None where no distance was seen."""
    out = []
    for j in range(len(arrays["steps"])):
        md = arrays["min_distance"][j]
        out.append({"episode_id": j, "min_distance": None if md == np.inf else md, "final_distance": arrays["final_distance"][j],
                    "steps": int(arrays["steps"][j]), "total_reward": arrays["total_reward"][j], "fuel_used": arrays["fuel_used"][j],
                    "lock_losses": int(arrays["lock_losses"][j]), "lock_recoveries": int(arrays["lock_recoveries"][j]),
                    "success": bool(arrays["success"][j])})
    return out


def aggregate_metrics(records) -> Dict[str, Any]:
    """_compute_aggregate_metrics (paper_benchmark_suite.py:366-398) over a list of episode dicts or a dict of record arrays.
    The reference reduces Python lists of numpy float32 scalars, i.e. float32 arrays; so does this, call for call."""
    if isinstance(records, dict):
        a = records
        succ = np.asarray(a["success"], bool)
        md = np.asarray(a["min_distance"], np.float32)
        md = md[md != np.inf]
        rew, fuel = np.asarray(a["total_reward"]), np.asarray(a["fuel_used"])
        steps, loss, rec = (np.asarray(a[k], np.int64) for k in ("steps", "lock_losses", "lock_recoveries"))
    else:
        succ = np.asarray([ep["success"] for ep in records])
        md = np.asarray([ep["min_distance"] for ep in records if ep["min_distance"] is not None])
        rew = np.asarray([ep["total_reward"] for ep in records])
        fuel = np.asarray([ep["fuel_used"] for ep in records])
        steps, loss, rec = (np.asarray([ep[k] for ep in records]) for k in ("steps", "lock_losses", "lock_recoveries"))
    some = md.size > 0
    return {
        "success_rate": float(np.mean(succ)),
        "success_rate_std": float(np.std(succ) / np.sqrt(len(succ))),      # SEM
        "mean_min_distance": float(np.mean(md)) if some else None,
        "std_min_distance": float(np.std(md)) if some else None,
        "median_min_distance": float(np.median(md)) if some else None,
        "best_min_distance": float(np.min(md)) if some else None,
        "mean_reward": float(np.mean(rew)),
        "std_reward": float(np.std(rew)),
        "mean_steps": float(np.mean(steps)),
        "mean_fuel_used": float(np.mean(fuel)),
        "mean_lock_losses": float(np.mean(loss)),
        "mean_lock_recoveries": float(np.mean(rec)),
        "lock_recovery_rate": float(np.sum(rec) / max(np.sum(loss), 1)),
        "sub_5m_rate": float(np.mean(md < 5)) if some else 0,
        "sub_10m_rate": float(np.mean(md < 10)) if some else 0,
        "sub_50m_rate": float(np.mean(md < 50)) if some else 0,
        "sub_100m_rate": float(np.mean(md < 100)) if some else 0,
    }


def _setup(n_episodes, config, n_envs, scenario_override):
    if int(n_episodes) < 1:
        raise ValueError(f"n_episodes must be >= 1 (got {n_episodes})")
    env_config = copy.deepcopy(dict(config or {}))
    if scenario_override:
        env_config.update(scenario_override)
    n = int(n_envs) if n_envs is not None else min(int(n_episodes), 65536)
    if n < 1:
        raise ValueError(f"n_envs must be >= 1 (got {n_envs})")
    # success threshold: the CONFIG DICT's proximity_kill_radius, default 50 (:286-287) -- not the environment's default of 20
    return env_config, n, math.ceil(int(n_episodes) / n), env_config.get("proximity_kill_radius", 50)


def _result(name, n_episodes, seed, ev, n):
    rec = ev.records()
    if int((rec["episodes"] >= ev.E).sum()) != n:
        raise RuntimeError(f"evaluation stopped with {int((rec['episodes'] >= ev.E).sum())} of {n} environments holding {ev.E} episodes")
    arrays = select_episodes(rec, int(n_episodes))
    res = {"policy_name": name, "n_episodes": int(n_episodes), "seed": seed,
           "episodes": episode_dicts(arrays) if int(n_episodes) <= EPISODE_DICTS_MAX else None}
    res.update(aggregate_metrics(arrays))
    res["records"] = arrays
    return res


def evaluate_classical_policy(policy, n_episodes: int, seed: int, config: Optional[Dict[str, Any]], n_envs: Optional[int] = None,
                              scenario_override: Optional[Dict[str, Any]] = None, device: int = 0, check_every: int = 64,
                              action_tape=None) -> Dict[str, Any]:
    """PolicyEvaluator.evaluate_classical_policy on the device.  `config`: the reference's environment config dict (e.g.
    scenarios.scenario_config(...)), updated with `scenario_override`.  n_envs environments (default min(n_episodes, 65536))
    run ceil(n_episodes / n_envs) episodes each; the law and the bookkeeping run in one kernel behind every step, the loop is
    issued from C and looks at the host every `check_every` steps.  Returns the reference's dict (policy_name, n_episodes,
    seed, episodes -- None beyond EPISODE_DICTS_MAX --, the aggregate keys) plus 'records': the kept episodes as arrays."""
    from .vec_env import HlynrVecEnv

    env_config, n, E, kill = _setup(n_episodes, config, n_envs, scenario_override)
    env = HlynrVecEnv(config=env_config, num_envs=n, device=device, seed=seed)
    ev = GuidanceEvaluator(n, policy, E, kill, device)
    try:
        ev.run(env, E * int(env.rc.max_steps), check_every, action_tape)
        return _result(policy.name, n_episodes, seed, ev, n)
    finally:
        ev.close()
        env.close()


def evaluate_policy(policy_fn: Callable, n_episodes: int, seed: int, config: Optional[Dict[str, Any]], n_envs: Optional[int] = None,
                    scenario_override: Optional[Dict[str, Any]] = None, device: int = 0, check_every: int = 64,
                    name: Optional[str] = None) -> Dict[str, Any]:
    """The same metrics for any callable `obs [N, 26] -> action [N, 6]` on device tensors (e.g. a deterministic PPO forward):
    the step runs through HlynrVecEnv.step_torch, the bookkeeping in the evaluation kernel without a law."""
    import torch

    from .vec_env import HlynrVecEnv

    env_config, n, E, kill = _setup(n_episodes, config, n_envs, scenario_override)
    env = HlynrVecEnv(config=env_config, num_envs=n, device=device, seed=seed)
    ev = GuidanceEvaluator(n, None, E, kill, device)
    try:
        obs = env.reset_torch()
        ev.begin(obs)
        with torch.no_grad():
            for t in range(E * int(env.rc.max_steps)):
                obs, rew, term, trunc, _ = env.step_torch(policy_fn(obs))
                ev.observe(obs, rew, term, trunc, env.terminal_obs, packed=env.info_packed)
                if (t + 1) % check_every == 0 and ev.done_count() >= n:
                    break
        return _result(name or getattr(policy_fn, "name", getattr(policy_fn, "__name__", type(policy_fn).__name__)), n_episodes, seed, ev, n)
    finally:
        ev.close()
        env.close()
