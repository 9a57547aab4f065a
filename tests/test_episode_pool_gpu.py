"""The next-episode pool's cooperative respawn (hlx_kernels.hip, lone-wave schedule) where its beam check DROPS entries.

A wave copies the prepared episodes of up to four finished lanes; the pass-1 beam check then drops the entries whose stored
beam test today's threshold decides differently (within 1e-5 of either threshold).  At the shipped beam widths (120 to 60
degrees) that never happens: a new episode looks straight at its missile (cosine ~1) or lies beyond radar range (cosine 2).
Here the beam is 0.2 degrees wide -- cos(0.1 deg) is within 1e-5 of 1, so every in-range entry is dropped -- and the radar
range (4.3 km) cuts the medium scenario's 3.1-5.5 km spawns about in half, so that dropped and kept entries share waves.
max_steps 19: whole waves finish in the same step.  Every check compares pool on with pool off bit for bit, and the last one
compares the pool-on kernel with the float64 oracle."""
import ctypes as C

import numpy as np
import pytest

from tests.philox_ref import philox4x32, u01

R_RADAR = 4300.0
NARROW = {"curriculum.radar_curriculum.initial_beam_width": 0.2, "curriculum.radar_curriculum.final_beam_width": 0.2,
          "radar.radar_range": R_RADAR, "max_steps": 19}
COOP_MAX = 4


def _cfg(physics="base", over=None):
    from hlynr_intercept_amd.scenarios import scenario_config
    return scenario_config("medium", physics, dict(NARROW, **(over or {})))


def _env(n, physics="base", over=None, seed=77, pool=1, radar_debug=False):
    from hlynr_intercept_amd.vec_env import HlynrVecEnv
    e = HlynrVecEnv(_cfg(physics, over), num_envs=n, seed=seed, radar_debug=radar_debug)
    e.set_load_schedule(2)            # the lone-wave schedule: the one the pool serves
    e.set_episode_pool(pool)
    return e


def _spawn_range(env):
    """Per environment: the distance at which the episode it holds now starts (inside radar range, its entry fails a 0.2 degree
    beam check; beyond it, the entry carries cosine 2 and passes)."""
    st = env.get_state()
    s = np.frombuffer(st, dtype=np.dtype(type(st[0])))
    ip, mp = s["int_pos"].astype(np.float32), s["mis_pos"].astype(np.float32)
    return np.linalg.norm((mp - ip).astype(np.float64), axis=1)


def _wave_triggers(done, dist, n):
    """(trigger waves, failing lanes in copy positions, waves with more than COOP_MAX finishes and a failing copy) of one step:
    a trigger is a whole wave in which, among its first COOP_MAX finished lanes, a failing lane comes before a passing one --
    the case the store loop used to hand the later lane the dropped lane's entry."""
    trig = fail = crowded = 0
    for b in range(n // 64):
        lanes = np.flatnonzero(done[64 * b:64 * b + 64])[:COOP_MAX]
        if lanes.size == 0:
            continue
        d = dist[64 * b + lanes]
        f, p = d < R_RADAR - 1.0, d > R_RADAR + 1.0      # (a metre of margin: no float32 rounding decides the class)
        fail += int(f.sum())
        if f.any() and p[int(np.argmax(f)):].any():
            trig += 1
        if int(done[64 * b:64 * b + 64].sum()) > COOP_MAX and f.any():
            crowded += 1
    return trig, fail, crowded


def _outputs(e, obs, rew, term, trunc):
    """Everything a step reports: observations, reward, flags, terminal observations, every info plane."""
    done = (term | trunc) != 0
    out = [obs.clone(), rew.clone(), term.clone(), trunc.clone(), e.terminal_obs[done].clone(), e.info_packed.clone()]
    for k, v in e.info.items():
        out.append(v[done].clone() if k in ("episode_return", "episode_length") else v.clone())
    return out


def _assert_same(ref, cur, what):
    import torch
    for k, (a, b) in enumerate(zip(ref, cur)):
        assert torch.equal(a, b), (what, k)


def _lockstep(envs, T, seed=12, ramp=None, count=True):
    """Step every env with the same actions; envs[0] (pool off) is the reference.  Returns the trigger statistics taken from
    the reference's post-step state."""
    import torch
    n = envs[0].num_envs
    for e in envs:
        if ramp is not None:
            e.set_training_step_count(ramp(0))
        e.reset_torch()
    g = torch.Generator(device=envs[0].device).manual_seed(seed)
    stats = dict(trig=0, fail=0, crowded=0, done=0)
    for t in range(T):
        a = torch.rand((n, 6), generator=g, device=envs[0].device) * 2 - 1
        if ramp is not None:
            for e in envs:
                e.set_training_step_count(ramp(t))
        ref = None
        for e in envs:
            cur = _outputs(e, *e.step_torch(a, want_done_list=True)[:4])
            if ref is None:
                ref = cur
            else:
                _assert_same(ref, cur, (t, e.episode_pool))
        done = ((ref[2] | ref[3]) != 0).cpu().numpy()
        stats["done"] += int(done.sum())
        if count and done.any():
            tr, f, c = _wave_triggers(done, _spawn_range(envs[0]), n)
            stats["trig"] += tr; stats["fail"] += f; stats["crowded"] += c
    s0 = bytes(envs[0].get_state())
    for e in envs[1:]:
        assert bytes(e.get_state()) == s0, e.episode_pool
    return stats


def test_narrow_beam_and_radar_range_split_the_spawns():
    """CPU, the oracle's reset from the auto-reset spawn draws of the seed the GPU tests use: the 4.3 km radar range puts
    between a third and two thirds of the new episodes inside the range, so dropped and kept entries share most waves,
    and an in-range episode looks at its missile within the margin of a 0.2 degree beam (its entry fails the check)."""
    import oracle.oracle as orc
    from hlynr_intercept_amd import _lib
    from hlynr_intercept_amd.config import resolve_config
    rc = resolve_config(_cfg())
    assert rc.radar_range == R_RADAR
    n, seed = 640, 77
    key = (seed & 0xFFFFFFFF, seed >> 32)
    fracs = []
    for ep in (1, 2, 3):
        rn = np.zeros((n, _lib.RESET_SLOTS))
        for i in range(n):
            w = [u01(x) for s in (8, 9, 10) for x in philox4x32((i, 0, ep, (0xFFFFFF << 8) | s), key)]
            rn[i, :10] = w[:10]
        ora = orc.OracleVec(rc, n)
        ora.reset(rn)
        ip, mp = ora.field("int_pos").astype(np.float32), ora.field("mis_pos").astype(np.float32)
        inr = np.linalg.norm((mp - ip).astype(np.float64), axis=1) <= R_RADAR
        fracs.append(inr.mean())
        # the interceptor points at its missile: the off-boresight angle is far inside the 1e-5 cosine margin
        q = ora.field("int_quat").astype(np.float64)
        w_, x_, y_, z_ = q.T
        fwd = np.stack([2 * (x_ * z_ + w_ * y_), 2 * (y_ * z_ - w_ * x_), 1 - 2 * (x_ * x_ + y_ * y_)], axis=1)   # body +Z
        los = (mp - ip).astype(np.float64)
        cosang = np.sum(fwd * los, axis=1) / np.linalg.norm(los, axis=1)
        assert np.all(np.abs(cosang - 1.0) < 1e-6), float(np.abs(cosang - 1.0).max())
        assert 1.0 - np.cos(np.radians(0.1)) < 1e-5
    assert all(0.33 < f < 0.67 for f in fracs), fracs


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1300, 1280])
def test_beam_check_drops_inside_a_wave_same_bits_as_no_pool(n):
    """Pool intervals 1, 8 and the default against pool off under the drop-inducing config: same bits at every step and in
    the final state; the trigger -- a failing lane ahead of a passing one among a wave's copied entries -- happened tens of
    times, and every failing copy was counted as a miss."""
    envs = [_env(n, pool=p) for p in (0, 1, 8, -1)]
    stats = _lockstep(envs, 80)
    assert stats["trig"] >= 20, stats
    assert envs[1].episode_pool_misses() >= stats["fail"] > 0, (envs[1].episode_pool_misses(), stats)
    assert envs[1].episode_pool_misses() < stats["done"]           # ... and the rest were copied
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_a_moving_narrow_ramp_drops_by_both_thresholds():
    """set_training_step_count at every step (as the reference's trainers call it), the beam width moving 0.05 -> 2 degrees
    and back across the ~0.5 degree edge below which every in-range entry is dropped: entries filled under one threshold are
    checked under the other, in both directions (today's threshold decides some drops, the entry's own threshold others)."""
    n, T = 1300, 120
    over = {"curriculum.radar_curriculum.initial_beam_width": 0.05, "curriculum.radar_curriculum.final_beam_width": 2.0,
            "curriculum.radar_curriculum.beam_width_transition_start": 0,
            "curriculum.radar_curriculum.beam_width_transition_end": 1000}
    period = 38                      # two episode lengths: an entry is filled one step after its episode starts, checked 18 later

    def ramp(t):                     # a triangle: 0 -> 1000 -> 0 over `period` steps, repeated
        p = t % period
        return int(1000 * (p if p < period // 2 else period - p) / (period // 2))

    from hlynr_intercept_amd.config import resolve_config
    rc = resolve_config(_cfg(over=over))
    beams = np.array([rc.radar_schedule(ramp(t))["beam_width"] for t in range(T)])
    off, on = _env(n, over=over, pool=0), _env(n, over=over, pool=1)
    # the batch truncates together at steps 18, 37, 56, ...; the entry used at step e was filled ahead of step e - 18 (the
    # first launch after its previous use), so its own threshold and today's lie on opposite sides of the edge, in both orders
    pairs = [(beams[e - 18], beams[e]) for e in range(18, T, 19)]
    assert any(a < 0.3 and b > 0.8 for a, b in pairs) and any(a > 0.8 and b < 0.3 for a, b in pairs), pairs
    stats = _lockstep([off, on], T, ramp=ramp)
    assert stats["trig"] > 0 and on.episode_pool_misses() > 0, stats
    off.close(); on.close()


WORD_CASES = [
    ("base", {}, False),
    ("v2dr", {}, False),                                      # thrust-lag and domain-randomisation state words
    ("v2", {}, False),                                        # onboard and ground delay rings (checked below)
    ("base", {"volley_mode": True, "volley_size": 2}, False),
    ("base", {"volley_mode": True, "volley_size": 3}, False),
    ("base", {"volley_mode": True, "volley_size": 4}, False),
    ("base", {}, True),                                       # radar_debug planes
]


@pytest.mark.gpu
@pytest.mark.parametrize("physics,over,radar_debug", WORD_CASES,
                         ids=["base", "v2dr", "v2-rings", "volley2", "volley3", "volley4", "radar_debug"])
def test_every_word_class_of_the_cooperative_store(physics, over, radar_debug):
    """st_word / on_word / gr_word / row_word of the cooperative store under drops, pool on against pool off."""
    from hlynr_intercept_amd.config import resolve_config
    rc = resolve_config(_cfg(physics, over))
    if physics == "v2":
        assert rc.onboard_delay > 0 and rc.ground_delay > 0, (rc.onboard_delay, rc.ground_delay)
    n = 1300
    envs = [_env(n, physics, over, pool=p, radar_debug=radar_debug) for p in (0, 1)]
    stats = _lockstep(envs, 60)
    assert stats["fail"] > 0, stats
    assert envs[1].episode_pool_misses() < stats["done"]
    for e in envs:
        e.close()


def _raw_step(e, a, terminal=True):
    from hlynr_intercept_amd import _lib as hl
    p = e._step_ptrs
    e._info_gen += 1
    hl.check(e._lib.hlx_step(e._h, a.data_ptr(), p[0], p[1], p[2], p[3], p[4] if terminal else None, None, None,
                             e._info_ref, e._stream()))


@pytest.mark.gpu
def test_without_terminal_observations():
    """The step without the terminal-observation output (and without the done list) under drops: same bits as pool off."""
    import torch
    n, T = 1300, 60
    envs = [_env(n, pool=p) for p in (0, 1)]
    for e in envs:
        e.reset_torch()
    g = torch.Generator(device=envs[0].device).manual_seed(4)
    for t in range(T):
        a = torch.rand((n, 6), generator=g, device=envs[0].device) * 2 - 1
        outs = []
        for e in envs:
            _raw_step(e, a, terminal=False)
            outs.append([e.obs.clone(), e.reward.clone(), e.terminated.clone(), e.truncated.clone(), e.info_packed.clone()])
        _assert_same(outs[0], outs[1], t)
    assert bytes(envs[0].get_state()) == bytes(envs[1].get_state())
    assert envs[1].episode_pool_misses() > 0
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_more_finishes_than_coop_max_with_drops():
    """Waves with five or more finishes where some of the first four fail: the rest compute in place (crowded), same bits."""
    n = 1280
    envs = [_env(n, pool=p, seed=5) for p in (0, 1)]
    stats = _lockstep(envs, 40, seed=3)
    assert stats["crowded"] > 0 and envs[1].episode_pool_crowded() > 0, (stats, envs[1].episode_pool_crowded())
    for e in envs:
        e.close()


@pytest.mark.gpu
def test_every_step_form_that_consumes_the_pool():
    """step_torch without the done list, the numpy step(), the separate info planes, the unfused rollout with several output
    slots and the guided evaluation run: pool on against pool off under drops."""
    import torch
    from hlynr_intercept_amd import _lib as hl
    from hlynr_intercept_amd import evaluation as ev_mod
    n, T = 1300, 60
    # step_torch without the done list
    a_off, a_on = _env(n, pool=0), _env(n, pool=1)
    for e in (a_off, a_on):
        e.reset_torch()
    g = torch.Generator(device=a_on.device).manual_seed(8)
    for t in range(T):
        a = torch.rand((n, 6), generator=g, device=a_on.device) * 2 - 1
        _assert_same(_outputs(a_off, *a_off.step_torch(a)[:4]), _outputs(a_on, *a_on.step_torch(a)[:4]), ("step_torch", t))
    assert bytes(a_off.get_state()) == bytes(a_on.get_state()) and a_on.episode_pool_misses() > 0
    a_off.close(); a_on.close()
    # the numpy step()
    b_off, b_on = _env(n, pool=0), _env(n, pool=1)
    for e in (b_off, b_on):
        e.reset()
    rng = np.random.default_rng(1)
    for t in range(T):
        a = rng.uniform(-1, 1, (n, 6)).astype(np.float32)
        (o0, r0, d0, i0), (o1, r1, d1, i1) = b_off.step(a), b_on.step(a)
        assert np.array_equal(o0, o1) and np.array_equal(r0, r1) and np.array_equal(d0, d1), t
        for (j, x), (k, y) in zip(i0.done_items(), i1.done_items()):
            assert j == k and np.array_equal(x["terminal_observation"], y["terminal_observation"]), t
            assert (x["episode"]["r"], x["episode"]["l"], x["distance"]) == (y["episode"]["r"], y["episode"]["l"], y["distance"]), t
    assert bytes(b_off.get_state()) == bytes(b_on.get_state())
    b_off.close(); b_on.close()
    # the separate info planes of the C ABI
    c_off, c_on = _env(n, pool=0), _env(n, pool=1)
    planes = []
    for e in (c_off, c_on):
        dev = e.device
        sep = dict(distance=torch.zeros(n, device=dev), min_distance=torch.zeros(n, device=dev), fuel=torch.zeros(n, device=dev),
                   fuel_used=torch.zeros(n, device=dev), flags=torch.zeros(n, dtype=torch.uint8, device=dev),
                   missiles=torch.zeros(n, dtype=torch.uint8, device=dev), interceptor_pos=torch.zeros((3, n), device=dev),
                   missile_pos=torch.zeros((3, n), device=dev), steps=torch.zeros(n, dtype=torch.int32, device=dev),
                   episode_return=torch.zeros(n, device=dev), episode_length=torch.zeros(n, dtype=torch.int32, device=dev))
        planes.append((sep, hl.HlxInfoSoa(**{k: v.data_ptr() for k, v in sep.items()})))
        e.reset_torch()
    g = torch.Generator(device=c_on.device).manual_seed(9)
    for t in range(T):
        a = torch.rand((n, 6), generator=g, device=c_on.device) * 2 - 1
        outs = []
        for e, (sep, soa) in zip((c_off, c_on), planes):
            p = e._step_ptrs
            hl.check(e._lib.hlx_step(e._h, a.data_ptr(), p[0], p[1], p[2], p[3], p[4], None, None, C.byref(soa), e._stream()))
            done = (e.terminated | e.truncated) != 0
            outs.append([e.obs.clone(), e.reward.clone(), e.terminated.clone(), e.truncated.clone(), e.terminal_obs[done].clone()] +
                        [v.clone() for v in sep.values()])
        _assert_same(outs[0], outs[1], ("separate planes", t))
    assert bytes(c_off.get_state()) == bytes(c_on.get_state()) and c_on.episode_pool_misses() > 0
    c_off.close(); c_on.close()
    # the unfused rollout, four output slots
    d_off, d_on = _env(n, pool=0), _env(n, pool=1)
    g = torch.Generator(device=d_on.device).manual_seed(10)
    tape = torch.rand((T, n, 6), generator=g, device=d_on.device) * 2 - 1
    ro = []
    for e in (d_off, d_on):
        e.reset_torch()
        e.set_rollout_fused(1)
        ro.append([x.clone() for x in e.rollout_torch(tape, 4)])
    _assert_same(ro[0], ro[1], "rollout")
    assert bytes(d_off.get_state()) == bytes(d_on.get_state()) and d_on.episode_pool_misses() > 0
    d_off.close(); d_on.close()
    # the guided evaluation run (hlx_eval_run): actions and records
    E, ms = 3, 19
    res = []
    for pool in (0, 1):
        e = _env(n, pool=pool)
        ev = ev_mod.GuidanceEvaluator(n, ev_mod.ProportionalNavigation(4.0, False), E, 50.0)
        act = torch.zeros((E * ms, n, 6), device=e.device)
        steps = ev.run(e, E * ms, 16, act)
        rec = ev.records()
        res.append((steps, act.cpu().numpy(), rec, e.episode_pool_misses()))
        ev.close(); e.close()
    (s0, a0, r0, _), (s1, a1, r1, m1) = res
    assert s0 == s1 and a0.tobytes() == a1.tobytes()
    for k in r0:
        assert r0[k].tobytes() == r1[k].tobytes(), k
    assert 0 < m1


@pytest.mark.gpu
def test_pool_on_kernel_matches_the_oracle():
    """The pool-on lone-wave kernel with in-kernel Philox draws (no noise buffers), running free, against the float64 oracle.
    The oracle's draws come from a noise-buffer twin of the same seed, which must also give the same bits; the bars are
    test_gpu_matches_oracle_free_running's."""
    import torch

    import oracle.oracle as orc
    from hlynr_intercept_amd.config import resolve_config
    from tests.test_gpu_parity import OBS_ATOL, RTOL, _check_reward_errors, _obs_err, _rel
    rc = resolve_config(_cfg())
    n, T = 1300, 80
    env, twin = _env(n, pool=1, seed=1234), _env(n, pool=0, seed=1234)
    ora = orc.OracleVec(rc, n)
    sn, rn = twin.fill_noise(for_reset=True)
    twin.set_noise(sn, rn)
    obs_g = env.reset_torch().clone()
    assert torch.equal(obs_g, twin.reset_torch())
    obs_o = ora.reset(rn.cpu().numpy().T.copy())
    assert np.max(_obs_err(obs_g.cpu().numpy(), obs_o)) <= OBS_ATOL
    g = torch.Generator(device="cpu").manual_seed(7)
    alive = np.ones(n, bool)
    worst = dict(obs=0.0, distance=0.0)
    rew_errs, n_done, trig = [], 0, 0
    for t in range(T):
        a = torch.rand((n, 6), generator=g) * 2 - 1
        if t % 3 == 0:
            a[:, 2] = 0.9
        sn, rn = twin.fill_noise()
        twin.set_noise(sn, rn)
        obs, rew, term, trunc, info = env.step_torch(a.to(env.device))
        tw = twin.step_torch(a.to(env.device))
        for x, y in zip((obs, rew, term, trunc), tw[:4]):
            assert torch.equal(x, y), t
        out = ora.step(a.numpy(), sn.cpu().numpy().T.copy(), rn.cpu().numpy().T.copy())
        term_h, trunc_h = term.cpu().numpy(), trunc.cpu().numpy()
        alive &= (term_h == out["terminated"]) & (trunc_h == out["truncated"]) & ((info["flags"].cpu().numpy() & 1) == out["intercepted"])
        done = (term_h | trunc_h).astype(bool)
        n_done += int(done.sum())
        obs_h = obs.cpu().numpy()
        step_obs_g = np.where(done[:, None], info["terminal_observation"].cpu().numpy(), obs_h)
        step_obs_o = np.where(done[:, None], ora.terminal_obs, out["obs"])
        eo = np.max(_obs_err(step_obs_g, step_obs_o), axis=1)
        alive &= eo <= 50 * OBS_ATOL
        worst["obs"] = max(worst["obs"], float(eo[alive].max(initial=0.0)))
        rew_errs.append(_rel(rew.cpu().numpy(), out["reward"])[alive])
        worst["distance"] = max(worst["distance"], float(_rel(info["distance"].cpu().numpy(), out["distance"])[alive].max(initial=0.0)))
        if done.any():
            sel = done & alive
            if sel.any():
                assert np.max(_obs_err(obs_h[sel], out["obs"][sel])) <= OBS_ATOL, t      # the copied first observations
            trig += _wave_triggers(done, _spawn_range(env), n)[0]
        fu_bad = info["fuel_used"].cpu().numpy() != out["fuel_used"]
        assert not fu_bad[alive].any(), (t, int(fu_bad.sum()))
    assert alive.all(), f"{(~alive).sum()} of {n} envs diverged in their discrete history"
    assert worst["obs"] <= OBS_ATOL and worst["distance"] <= RTOL, worst
    _check_reward_errors(np.concatenate(rew_errs), rc, "pool on")
    st = env.get_state()
    for name in ("int_pos", "int_vel", "int_quat", "mis_pos", "mis_vel", "wind"):
        mine = np.array([list(getattr(st[i], name)) for i in range(n)])
        assert np.max(_rel(mine, ora.field(name))) <= 2 * RTOL, name
    kx = np.array([list(st[i].kf_x) for i in range(n)])
    assert float(np.max(_rel(kx[:, :3], ora.field("kf_x")[:, :3]))) <= 1e-6
    P = np.array([list(st[i].kf_P) for i in range(n)])
    Po = ora.field("kf_P").reshape(n, 6, 6)
    Pref = np.stack([Po[:, 0, 0], Po[:, 0, 3], Po[:, 3, 0], Po[:, 3, 3]], axis=1)
    assert float(np.max(np.abs(P - Pref) / np.maximum(1e-2, np.abs(Pref)))) <= 1e-6
    assert np.array_equal(np.array([st[i].steps for i in range(n)]), ora.field("steps"))
    assert bytes(st) == bytes(twin.get_state())
    # the pool really served this run, and the drop-before-keep case was among what it served
    assert env.episode_pool_misses() < n_done and trig > 0, (env.episode_pool_misses(), n_done, trig)
    env.close(); twin.close()
