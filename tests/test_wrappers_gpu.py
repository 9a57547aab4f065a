"""On-device VecFrameStack + VecNormalize (include/hlx_obs.h, hlynr_intercept_amd/wrappers.py) against the numpy
restatement of the SB3 wrappers (oracle/vec_wrappers.py), fed with the raw step outputs of an identically seeded
un-wrapped environment.  Tolerances: the raw stacks are bit-exact; normalised values agree to 1e-5 relative
(float64 statistics on both sides; the GPU multiplies by a float64 reciprocal where numpy divides)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RTOL, ATOL = 1e-5, 2e-6


def _make(n, seed=9, max_steps=23):
    from hlynr_intercept_amd.scenarios import scenario_config
    from hlynr_intercept_amd.vec_env import HlynrVecEnv
    return HlynrVecEnv(scenario_config("medium", "base", {"max_steps": max_steps}), num_envs=n, seed=seed)


def _raw_trace(n, T, seed=9):
    """Raw (obs0, [obs, reward, done, terminal_obs] per step, actions) of the un-wrapped environment."""
    import torch
    env = _make(n, seed)
    g = torch.Generator(device=env.device).manual_seed(4)
    acts = torch.rand((T, n, 6), generator=g, device=env.device) * 2 - 1
    obs0 = env.reset_torch().cpu().numpy().copy()
    steps = []
    for t in range(T):
        o, r, te, tr, info = env.step_torch(acts[t])
        steps.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), ((te | tr) != 0).cpu().numpy(),
                      info["terminal_observation"].cpu().numpy().copy()))
    env.close()
    return obs0, steps, acts


@pytest.mark.parametrize("n,n_stack,norm_reward", [(257, 4, False), (64, 1, True), (1000, 3, True)])
def test_stack_and_normalize_match_the_sb3_restatement(n, n_stack, norm_reward):
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    from oracle.vec_wrappers import FrameStack, Normalize
    T = 70
    obs0, steps, acts = _raw_trace(n, T)
    env = _make(n)
    wrapped = VecNormalize(VecFrameStack(env, n_stack=n_stack) if n_stack > 1 else env, norm_obs=True,
                           norm_reward=norm_reward, clip_obs=10.0, clip_reward=10.0, gamma=0.99)
    assert wrapped.observation_space.shape == (26 * n_stack,)
    fs, nz = FrameStack(n, 26, n_stack), Normalize(n, 26 * n_stack, norm_reward=norm_reward)
    nz32 = Normalize(n, 26 * n_stack, norm_reward=norm_reward, batch_f32=True)   # SB3's float32 batch moments
    fs32 = FrameStack(n, 26, n_stack)
    got = wrapped.reset_torch().cpu().numpy()
    want = nz.reset(fs.reset(obs0))
    nz32.reset(fs32.reset(obs0))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)
    n_done, worst32 = 0, 0.0
    for t in range(T):
        o, r, te, tr, info = wrapped.step_torch(acts[t])
        raw_o, raw_r, done, raw_term = steps[t]
        stacked, term_stacked = fs.step(raw_o, done, raw_term)
        want_o, want_r, want_t = nz.step(stacked, raw_r, done, term_stacked)
        s32, t32 = fs32.step(raw_o, done, raw_term)
        o32, _, _ = nz32.step(s32, raw_r, done, t32)
        got_o = o.cpu().numpy()
        assert np.array_equal(((te | tr) != 0).cpu().numpy(), done)
        np.testing.assert_allclose(got_o, want_o, rtol=RTOL, atol=ATOL, err_msg=f"step {t}")
        np.testing.assert_allclose(r.cpu().numpy(), want_r, rtol=RTOL, atol=ATOL, err_msg=f"reward step {t}")
        assert np.array_equal(wrapped.get_original_obs(), stacked)                 # raw stacks: bit-exact
        assert np.array_equal(info["original_reward"].cpu().numpy(), raw_r)
        if done.any():
            n_done += int(done.sum())
            np.testing.assert_allclose(info["terminal_observation"].cpu().numpy()[done], want_t[done], rtol=RTOL, atol=ATOL)
        worst32 = max(worst32, float(np.abs(got_o - o32).max()))
    assert n_done >= 2 * n                                                          # several resets per env (max_steps 23)
    np.testing.assert_allclose(wrapped.obs_rms.mean, nz.obs_rms.mean, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(wrapped.obs_rms.var, nz.obs_rms.var, rtol=1e-9, atol=1e-12)
    assert wrapped.obs_rms.count == pytest.approx(nz.obs_rms.count, rel=1e-12)
    np.testing.assert_allclose(wrapped.ret_rms.mean, nz.ret_rms.mean, rtol=1e-9)
    np.testing.assert_allclose(wrapped.ret_rms.var, nz.ret_rms.var, rtol=1e-9)
    # float32 batch moments (what SB3 itself accumulates) move the normalised values by far less than the clip range
    assert worst32 < 5e-3
    wrapped.close()


def test_frame_stack_alone_is_bit_exact_and_eval_mode_freezes_statistics(tmp_path):
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    from oracle.vec_wrappers import FrameStack
    n, T = 130, 40
    obs0, steps, acts = _raw_trace(n, T)
    env = _make(n)
    st = VecFrameStack(env, n_stack=4)
    fs = FrameStack(n, 26, 4)
    assert np.array_equal(st.reset_torch().cpu().numpy(), fs.reset(obs0))
    for t in range(T):
        o, r, te, tr, info = st.step_torch(acts[t])
        stacked, term = fs.step(steps[t][0], steps[t][2], steps[t][3])
        assert np.array_equal(o.cpu().numpy(), stacked)
        assert np.array_equal(r.cpu().numpy(), steps[t][1])
        d = steps[t][2]
        assert np.array_equal(info["terminal_observation"].cpu().numpy()[d], term[d])
    st.close()

    # VecNormalize: save -> load into a fresh env -> evaluation mode keeps the statistics and normalises identically
    env = _make(n)
    vn = VecNormalize(VecFrameStack(env, n_stack=4), norm_reward=False)
    vn.reset_torch()
    for t in range(10):
        vn.step_torch(acts[t])
    path = str(tmp_path / "vec_normalize.pkl")
    vn.save(path)
    mean, var, count = vn.obs_rms.mean.copy(), vn.obs_rms.var.copy(), vn.obs_rms.count
    vn.training = False
    o_eval = vn.step_torch(acts[10])[0].cpu().numpy().copy()
    assert np.array_equal(vn.obs_rms.mean, mean) and vn.obs_rms.count == count
    raw = vn.get_original_obs()
    np.testing.assert_allclose(o_eval, vn.normalize_obs(raw), rtol=RTOL, atol=ATOL)
    vn.close()
    env2 = _make(n)
    vn2 = VecNormalize.load(path, VecFrameStack(env2, n_stack=4))
    assert np.array_equal(vn2.obs_rms.mean, mean) and np.array_equal(vn2.obs_rms.var, var) and vn2.obs_rms.count == count
    vn2.training = False
    vn2.reset_torch()
    for t in range(11):
        o2 = vn2.step_torch(acts[t])[0]
    np.testing.assert_allclose(o2.cpu().numpy(), o_eval, rtol=RTOL, atol=ATOL)     # same env seed, same frozen statistics
    vn2.close()


def test_sb3_numpy_contract_of_the_wrapped_env():
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    n = 48
    env = VecNormalize(VecFrameStack(_make(n, max_steps=12), n_stack=4), norm_obs=True, norm_reward=False, clip_obs=10.0)
    obs = env.reset()
    assert obs.shape == (n, 104) and obs.dtype == np.float32
    rng = np.random.default_rng(0)
    seen_done = False
    for t in range(30):
        obs, rew, dones, infos = env.step(rng.uniform(-1, 1, (n, 6)).astype(np.float32))
        assert obs.shape == (n, 104) and rew.shape == (n,) and dones.shape == (n,) and len(infos) == n
        assert np.abs(obs).max() <= 10.0
        for i, info in infos.done_items():
            seen_done = True
            assert info["terminal_observation"].shape == (104,) and "episode" in info
    assert seen_done
    env.env_method("set_training_step_count", 1234)                                 # passes through to the base env
    assert env.get_attr("observation_generator")[0].radar_beam_width > 0
    env.close()


@pytest.mark.parametrize("n,n_stack", [(4099, 4), (300, 2), (70, 8), (9000, 4)])
def test_incremental_moments_equal_the_full_reduction(n, n_stack):
    """Step pushes that follow a training push reduce only the newest frame and subtract the frames of the environments
    that were reset.  By default the step kernel itself writes the newest frame's partial sums and
    hlx_obs_finalize_fused_kernel subtracts the leaving frames; HLX_OBS_NO_FUSE=1 takes the same incremental sums from
    hlx_obs_moments_inc_kernel instead; HLX_OBS_FULL_MOMENTS=1 forces the full reduction over all n_stack frames.
    Same batches, all three ways: the running statistics agree to float64 rounding, including across eval-mode gaps."""
    import torch
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    T = 90
    stats = {}
    for form in ("fused", "full", "no_fuse"):
        full = form == "full"
        env_var = {"fused": None, "full": "HLX_OBS_FULL_MOMENTS", "no_fuse": "HLX_OBS_NO_FUSE"}[form]
        if env_var:
            os.environ[env_var] = "1"
        try:
            w = VecNormalize(VecFrameStack(_make(n, seed=21, max_steps=17), n_stack), norm_reward=True)
            g = torch.Generator(device=w.device).manual_seed(8)
            acts = torch.rand((T, n, 6), generator=g, device=w.device) * 2 - 1
            w.reset_torch()
            snaps = []
            for t in range(T):
                if t == 40:
                    w.training = False          # statistics frozen: the next training push must fall back to the full form
                if t == 47:
                    w.training = True
                w.step_torch(acts[t])
                if t % 10 == 9:
                    snaps.append((w.obs_rms.mean.copy(), w.obs_rms.var.copy(), w.obs_rms.count, w.ret_rms.var))
            stats[full if form != "no_fuse" else form] = snaps
            w.close()
        finally:
            if env_var:
                os.environ.pop(env_var, None)
    for (m0, v0, c0, r0), (m1, v1, c1, r1) in zip(stats[False], stats[True]):
        # (the return sums: identical order in the incremental and the full kernel; one more order since round 3, when the step
        # kernel forms them per 64-environment block -- float64 rounding apart)
        assert c0 == c1 and abs(r0 - r1) <= 1e-13 * max(1.0, abs(r1))
        assert np.max(np.abs(m0 - m1)) <= 1e-12 * max(1.0, np.max(np.abs(m1)))
        assert np.max(np.abs(v0 - v1)) <= 1e-11 * max(1.0, np.max(np.abs(v1)))
    assert len(stats["no_fuse"]) == len(stats[True])
    for (m0, v0, c0, r0), (m1, v1, c1, r1) in zip(stats["no_fuse"], stats[True]):
        assert c0 == c1 and abs(r0 - r1) <= 1e-13 * max(1.0, abs(r1))
        assert np.max(np.abs(m0 - m1)) <= 1e-12 * max(1.0, np.max(np.abs(m1)))
        assert np.max(np.abs(v0 - v1)) <= 1e-11 * max(1.0, np.max(np.abs(v1)))
    assert stats[False][-1][2] > n * 70      # the statistics did advance


def test_a_file_sb3_itself_wrote_loads_into_the_device_pipeline_or_is_refused_by_shape(tmp_path):
    """tests/golden/sb3/vec_normalize_final.pkl (written by Stable-Baselines3 for the reference's legacy 17-D environment):
    `VecNormalize.load` refuses it on the 26-D environment, as SB3's own `set_venv` does (check_shape_equal); with its
    statistics widened to 26 columns the load -> step in evaluation mode -> save -> read chain keeps every number."""
    from hlynr_intercept_amd.wrappers import VecNormalize, read_vecnormalize_pickle, write_vecnormalize_pickle
    genuine = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sb3", "vec_normalize_final.pkl")
    d = read_vecnormalize_pickle(genuine)
    env = _make(130)
    with pytest.raises(ValueError):
        VecNormalize.load(genuine, env)
    env.close()
    wide = dict(d, format="hlynr-vecnormalize-v1", n_stack=1, training=False,
                obs_mean=np.concatenate([d["obs_mean"], d["obs_mean"][:9]]), obs_var=np.concatenate([d["obs_var"], d["obs_var"][:9]]))
    p, q = str(tmp_path / "wide.pkl"), str(tmp_path / "saved.pkl")
    write_vecnormalize_pickle(p, wide, None, None, 130)
    env = _make(130)
    v = VecNormalize.load(p, env)
    assert v.training is False and v.norm_reward is True and v.clip_obs == 10.0 and v.gamma == 0.99
    import torch
    o = v.reset_torch().cpu().numpy()
    raw = v.get_original_obs()
    want = np.clip((raw.astype(np.float64) - wide["obs_mean"]) / np.sqrt(wide["obs_var"] + 1e-8), -10.0, 10.0)
    assert np.allclose(o, want, rtol=RTOL, atol=ATOL)
    v.step_torch(torch.zeros((130, 6), device=env.device))          # evaluation mode: the statistics must not move
    v.save(q)
    back = read_vecnormalize_pickle(q)
    for k in ("obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "clip_obs", "clip_reward", "gamma", "epsilon",
              "norm_obs", "norm_reward", "training"):
        assert np.array_equal(back[k], wide[k]), k
    v.close()

