"""Every dispatch branch of the on-device observation pipeline (include/hlx_obs.h, csrc/hlx_obs.inc) against the float64
numpy restatement of SB3's VecFrameStack / VecNormalize (oracle/vec_wrappers.py).

A. The standalone C ABI (hlx_obs_push_reset / hlx_obs_push / hlx_obs_emit / hlx_obs_set_stats) with frames the test makes,
   over a (D, n_stack) grid that reaches the scalar, pair and incremental moments kernels and the three emit kernels.
B. The three moment forms (fused into the step kernel, HLX_OBS_NO_FUSE=1 -> incremental kernel, HLX_OBS_FULL_MOMENTS=1) through
   the real step, under four physics variants and the three load schedules; the noise-buffer route to the incremental kernel.
C. Batches above the 1 024-block cap of the moments kernels, and both sides of the 4 GiB store boundary of the rows emit.
D. Determinism (fixed-order reductions) and the conditioning of the one-pass batch variance.

Bounds (the same as tests/test_wrappers_gpu.py): raw stacks bit-exact; normalised observations and rewards rtol 1e-5,
atol 2e-6; running mean / variance rtol 1e-9; counts 1e-12."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RTOL, ATOL = 1e-5, 2e-6
STAT_RTOL, STAT_ATOL, COUNT_REL = 1e-9, 1e-12, 1e-12
MEMCPY_D2D = 3     # hipMemcpyDeviceToDevice


class _Pipe:
    """One hlx_obs pipeline driven through the C ABI.  Frames are copied into hlx_obs_next_slot() with hipMemcpyAsync on
    torch's current stream (the HIP runtime libhlx.so resolves, i.e. the one torch loaded), where every launch goes too."""

    def __init__(self, n, D, S, training=True, norm_obs=True, norm_reward=True, clip_obs=5.0, clip_reward=10.0, gamma=0.9,
                 epsilon=1e-4, outputs=True):
        import torch
        from hlynr_intercept_amd import _lib
        self.torch, self._lib = torch, _lib
        self.lib = _lib.load()
        self.n, self.D, self.S, self.F = n, D, S, D * S
        self.cfg = _lib.HlxObsConfig(n_envs=n, obs_dim=D, n_stack=S, device=0, norm_obs=int(norm_obs), norm_reward=int(norm_reward),
                                     training=int(training), clip_obs=clip_obs, clip_reward=clip_reward, gamma=gamma, epsilon=epsilon)
        self.p = C.c_void_p()
        _lib.check(self.lib.hlx_obs_create(C.byref(self.cfg), C.byref(self.p)))
        assert self.lib.hlx_obs_feature_dim(self.p) == self.F
        self.dev = torch.device("cuda", 0)
        self.memcpy = self.lib.hipMemcpyAsync
        self.memcpy.restype, self.memcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.out = torch.zeros((n, self.F), dtype=torch.float32, device=self.dev)
        if outputs:
            self.term_out = torch.zeros((n, self.F), dtype=torch.float32, device=self.dev)
            self.rew_out = torch.zeros(n, dtype=torch.float32, device=self.dev)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def write(self, frames):
        """frames: contiguous float32 [n, D] device tensor -> the ring slot of the next push."""
        assert frames.dtype == self.torch.float32 and frames.is_contiguous() and tuple(frames.shape) == (self.n, self.D)
        dst = self.lib.hlx_obs_next_slot(self.p)
        assert dst
        assert self.memcpy(dst, frames.data_ptr(), frames.numel() * 4, MEMCPY_D2D, self.stream()) == 0

    def dptr(self, x):
        return None if x is None else x.data_ptr()

    def push_reset(self, frames):
        self.write(frames)
        self._lib.check(self.lib.hlx_obs_push_reset(self.p, self.out.data_ptr(), self.stream()))

    def push(self, frames, term, trunc, terminal_obs, reward, term_out=True, rew_out=True):
        self.write(frames)
        self._lib.check(self.lib.hlx_obs_push(self.p, self.dptr(term), self.dptr(trunc), self.dptr(terminal_obs), self.dptr(reward),
                                              self.out.data_ptr(), self.term_out.data_ptr() if term_out else None,
                                              self.rew_out.data_ptr() if rew_out else None, self.stream()))

    def emit(self, normalise):
        o = self.torch.zeros_like(self.out)
        self._lib.check(self.lib.hlx_obs_emit(self.p, int(normalise), o.data_ptr(), self.stream()))
        return o.cpu().numpy()

    def set_mode(self, training, norm_obs, norm_reward):
        self._lib.check(self.lib.hlx_obs_set_mode(self.p, int(training), int(norm_obs), int(norm_reward)))

    def stats(self):
        mean, var, sc = np.zeros(self.F), np.zeros(self.F), (C.c_double * 4)()
        self._lib.check(self.lib.hlx_obs_get_stats(self.p, mean.ctypes.data, var.ctypes.data, C.addressof(sc)))
        return mean, var, list(sc)

    def set_stats(self, mean, var, scalars):
        mean, var = np.ascontiguousarray(mean, np.float64), np.ascontiguousarray(var, np.float64)
        sc = (C.c_double * 4)(*scalars)
        self._lib.check(self.lib.hlx_obs_set_stats(self.p, mean.ctypes.data, var.ctypes.data, C.addressof(sc)))

    def close(self):
        if self.p:
            self.torch.cuda.synchronize(self.dev)
            self._lib.check(self.lib.hlx_obs_destroy(self.p))
            self.p = C.c_void_p()


def _check_stats(pipe, nz, what):
    mean, var, sc = pipe.stats()
    np.testing.assert_allclose(mean, nz.obs_rms.mean, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"obs mean {what}")
    np.testing.assert_allclose(var, nz.obs_rms.var, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"obs var {what}")
    assert sc[0] == pytest.approx(nz.obs_rms.count, rel=COUNT_REL), what
    assert sc[3] == pytest.approx(nz.ret_rms.count, rel=COUNT_REL), what
    np.testing.assert_allclose(sc[1], nz.ret_rms.mean, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"ret mean {what}")
    np.testing.assert_allclose(sc[2], nz.ret_rms.var, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"ret var {what}")
    return mean, var, sc


class _Frames:
    """Synthetic frames: per-column scales 1e-2 / 1 / 1e2 (magnitudes 1e4 apart), the last column constant (D >= 3), a few
    outliers far beyond clip_obs standard deviations."""

    def __init__(self, n, D, seed):
        self.rng = np.random.default_rng(seed)
        self.n, self.D = n, D
        self.scale = np.array([(1e-2, 1.0, 1e2)[j % 3] for j in range(D)])
        self.offset = 0.5 * self.scale * np.array([(-1.0) ** j for j in range(D)])

    def __call__(self):
        x = self.offset + self.scale * self.rng.standard_normal((self.n, self.D))
        out = self.rng.random((self.n, self.D)) < 0.01
        x[out] *= 60.0
        if self.D >= 3:
            x[:, -1] = 0.75
        return x.astype(np.float32)


def _flags(rng, n, p):
    return rng.random(n) < p


def _run_case(n, D, S, seed=0, record=None, early_all_done=False):
    """The push sequence of section A on one pipeline, each push checked against the oracle.  `record`: a list that receives
    (outputs, statistics) of every push, for the determinism test.  `early_all_done`: every environment finishes on the sixth
    push, before an 8-deep stack has filled (test_a_never_filled_stack_position_that_empties_incrementally)."""
    import torch
    from oracle.vec_wrappers import FrameStack, Normalize
    dev = torch.device("cuda", 0)
    cfg = dict(clip_obs=5.0, clip_reward=10.0, gamma=0.9, epsilon=1e-4)
    pipe = _Pipe(n, D, S, training=True, norm_obs=True, norm_reward=True, **cfg)
    fs = FrameStack(n, D, S)
    nz = Normalize(n, D * S, training=True, norm_obs=True, norm_reward=True, **cfg)
    gen, rng = _Frames(n, D, seed), np.random.default_rng(seed + 1)
    tdev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u8 = lambda a: tdev(a.astype(np.uint8))                              # noqa: E731

    def rec(*xs):
        if record is not None:
            record.append(tuple(np.array(x, copy=True) for x in xs) + tuple(np.array(s, copy=True) for s in pipe.stats()[:2]))

    def cmp_obs(got, want, what):
        if nz.norm_obs:
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)
        else:
            assert np.array_equal(got, want), what                       # raw stacks: bit-exact

    def reset(what):
        f = gen()
        pipe.push_reset(tdev(f))
        want = nz.reset(fs.reset(f))
        got = pipe.out.cpu().numpy()
        cmp_obs(got, want, what)
        _check_stats(pipe, nz, what)
        rec(got)

    def step(what, term=None, trunc=None, terminal=True, reward=True, term_out=True, rew_out=True):
        f = gen()
        tob = gen() if terminal else None
        rw = (3.0 * rng.standard_normal(n)).astype(np.float32) if reward else None
        dones = np.zeros(n, bool)
        for x in (term, trunc):
            if x is not None:
                dones |= x
        pipe.push(tdev(f), None if term is None else u8(term), None if trunc is None else u8(trunc),
                  None if tob is None else tdev(tob), None if rw is None else tdev(rw), term_out=term_out, rew_out=rew_out)
        stacked, term_stacked = fs.step(f, dones, tob if tob is not None else np.zeros((n, D), np.float32))
        want_o, want_r, want_t = nz.step(stacked, rw, dones, term_stacked)
        got = pipe.out.cpu().numpy()
        cmp_obs(got, want_o, what)
        if tob is not None and term_out and dones.any():
            cmp_obs(pipe.term_out.cpu().numpy()[dones], want_t[dones], what + " terminal")
        if rw is not None and rew_out:
            got_r = pipe.rew_out.cpu().numpy()
            if nz.norm_reward:
                np.testing.assert_allclose(got_r, want_r, rtol=RTOL, atol=ATOL, err_msg=what + " reward")
            else:
                assert np.array_equal(got_r, rw), what + " reward"
        _check_stats(pipe, nz, what)
        rec(got)
        return stacked

    def emits(stacked, what):
        assert np.array_equal(pipe.emit(0), stacked), what + " emit(0)"
        mean, var = nz.obs_rms.mean, nz.obs_rms.var
        want = np.clip((stacked - mean) / np.sqrt(var + nz.epsilon), -nz.clip_obs, nz.clip_obs).astype(np.float32)
        np.testing.assert_allclose(pipe.emit(1), want, rtol=RTOL, atol=ATOL, err_msg=what + " emit(1)")

    def mode(training, norm_obs, norm_reward):
        pipe.set_mode(training, norm_obs, norm_reward)
        nz.training, nz.norm_obs, nz.norm_reward = training, norm_obs, norm_reward

    every = np.ones(n, bool)
    first = np.zeros(n, bool)
    first[0] = True
    try:
        reset("reset")
        t = _flags(rng, n, 0.15) | first
        step("terminated only", term=t)
        step("truncated only, env 0 again", trunc=_flags(rng, n, 0.15) | first)
        te, tr = _flags(rng, n, 0.2), _flags(rng, n, 0.2)
        step("both flags", term=te, trunc=tr)
        step("no flags")                                                   # both pointers NULL
        step("reward NULL, terminal_obs NULL", term=_flags(rng, n, 0.2), terminal=False, reward=False)
        if not early_all_done:
            for k in range(3):                                             # every stack position has held a frame
                step(f"incremental {k}", term=_flags(rng, n, 0.1))
        s = step("every environment", term=every, term_out=False, rew_out=False)
        emits(s, "after all finished")
        step("env 0 right after its reset", trunc=first)
        step("incremental", term=_flags(rng, n, 0.1))
        reset("second reset")
        step("env 0 right after the second reset", term=first | _flags(rng, n, 0.1))
        s = step("incremental 2", trunc=_flags(rng, n, 0.1))
        emits(s, "mid-run")
        mode(False, True, True)
        step("evaluation", term=_flags(rng, n, 0.2))
        step("evaluation 2", trunc=_flags(rng, n, 0.2))
        mode(True, True, True)
        step("training again: full reduction", term=_flags(rng, n, 0.1))
        step("incremental 3", term=_flags(rng, n, 0.1))
        mode(True, False, True)
        step("norm_obs off, training on", term=_flags(rng, n, 0.1))
        mode(True, True, False)
        step("norm_reward off", trunc=_flags(rng, n, 0.1))
        s = step("incremental 4", term=_flags(rng, n, 0.1), trunc=_flags(rng, n, 0.05))
        emits(s, "late")
        # statistics loaded from outside (VecNormalize.load)
        F = D * S
        lm = np.linspace(-2.0, 3.0, F)
        lv = np.linspace(0.5, 40.0, F)
        pipe.set_stats(lm, lv, [123.0, 0.25, 7.5, 456.0])
        nz.obs_rms.mean, nz.obs_rms.var, nz.obs_rms.count = lm.copy(), lv.copy(), 123.0
        nz.ret_rms.mean, nz.ret_rms.var, nz.ret_rms.count = 0.25, 7.5, 456.0
        _check_stats(pipe, nz, "set_stats")
        emits(s, "after set_stats")
        mode(True, True, True)
        step("after set_stats", term=_flags(rng, n, 0.1))
        step("after set_stats 2", trunc=_flags(rng, n, 0.1))
    finally:
        pipe.close()


# (D, n_stack): what each case reaches -- moments kernel / emit kernel
GRID = [
    (1, 1),      # scalar (256 threads)          emit<1>
    (1, 8),      # scalar                        emit<4>
    (7, 3),      # scalar, 252 threads           emit<1>
    (7, 4),      # scalar                        emit<4>
    (255, 1),    # scalar, 255 threads           emit<1>
    (2, 2),      # pair / incremental, H 1       rows, one chunk
    (26, 3),     # pair / incremental            emit<1>
    (26, 4),     # pair / incremental            rows
    (130, 2),    # pair / incremental, H 65, R 3  rows, 65 chunks
    (256, 4),    # pair / incremental, H 128, R 2 rows at F/4 = 256
    (256, 8),    # pair / incremental            emit<4> (F/4 > 256)
]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("D,S", GRID)
def test_c_abi_push_sequence_matches_the_oracle(D, S, n):
    _run_case(n, D, S, seed=D * 131 + S * 7 + n)


@pytest.mark.xfail(strict=True, reason="known: the incremental forms give a stack position's batch sums as (last push's sums) - "
                   "(sums of the rows that leave); a position that held no frame until the last push and is emptied by this one "
                   "keeps a rounding residue of ~1e-16 x the leaving sum of squares instead of an exact 0, which moves its tiny "
                   "running variance (~1e-7) by ~1e-10 (relative 1e-3)")
def test_a_never_filled_stack_position_that_empties_incrementally():
    _run_case(1000, 256, 8, seed=256 * 131 + 8 * 7 + 1000, early_all_done=True)


@pytest.mark.parametrize("D,S", [(7, 3), (2, 2)])
def test_c_abi_above_the_moments_block_cap(D, S):
    """n = 70 001: 1 094 environment blocks of 64, the moments kernels' grid capped at 1 024 blocks."""
    _run_case(70001, D, S, seed=5)


# ----------------------------------------------------------------------------------------------------------------- B
def _make_env(preset, n, seed, schedule, max_steps=13):
    from hlynr_intercept_amd.scenarios import scenario_config
    from hlynr_intercept_amd.vec_env import HlynrVecEnv
    scen, phys, extra = preset
    env = HlynrVecEnv(scenario_config(scen, phys, dict(extra, max_steps=max_steps)), num_envs=n, seed=seed)
    if schedule is not None:
        env.set_load_schedule(schedule)
        assert env.load_schedule == schedule
    return env


def _raw_trace(preset, n, T, seed, schedule, noise=False, max_steps=13):
    import torch
    env = _make_env(preset, n, seed, schedule, max_steps)
    g = torch.Generator(device=env.device).manual_seed(4)
    acts = torch.rand((T, n, 6), generator=g, device=env.device) * 2 - 1
    if noise:
        env.set_noise(*env.fill_noise(for_reset=True))
    obs0 = env.reset_torch().cpu().numpy().copy()
    steps = []
    for t in range(T):
        if noise:
            env.set_noise(*env.fill_noise())
        o, r, te, tr, info = env.step_torch(acts[t])
        steps.append((o.cpu().numpy().copy(), r.cpu().numpy().copy(), ((te | tr) != 0).cpu().numpy(),
                      info["terminal_observation"].cpu().numpy().copy()))
    env.close()
    return obs0, steps, acts


def _wrapped_run(preset, n, T, seed, schedule, trace, env_var=None, noise=False, n_stack=4, max_steps=13, snapshots=None):
    """VecNormalize(VecFrameStack(env, n_stack), norm_reward=True) against the oracle, every step."""
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    from oracle.vec_wrappers import FrameStack, Normalize
    obs0, steps, acts = trace
    if env_var:
        os.environ[env_var] = "1"
    try:
        env = _make_env(preset, n, seed, schedule, max_steps)
        w = VecNormalize(VecFrameStack(env, n_stack=n_stack), norm_obs=True, norm_reward=True, clip_obs=10.0, clip_reward=10.0, gamma=0.99)
        F = 26 * n_stack
        fs, nz = FrameStack(n, 26, n_stack), Normalize(n, F, norm_reward=True)
        if noise:
            env.set_noise(*env.fill_noise(for_reset=True))
        np.testing.assert_allclose(w.reset_torch().cpu().numpy(), nz.reset(fs.reset(obs0)), rtol=RTOL, atol=ATOL)
        n_done = 0
        for t in range(T):
            if noise:
                env.set_noise(*env.fill_noise())
            o, r, te, tr, info = w.step_torch(acts[t])
            raw_o, raw_r, done, raw_term = steps[t]
            stacked, term_stacked = fs.step(raw_o, done, raw_term)
            want_o, want_r, want_t = nz.step(stacked, raw_r, done, term_stacked)
            assert np.array_equal(((te | tr) != 0).cpu().numpy(), done), t
            np.testing.assert_allclose(o.cpu().numpy(), want_o, rtol=RTOL, atol=ATOL, err_msg=f"step {t}")
            np.testing.assert_allclose(r.cpu().numpy(), want_r, rtol=RTOL, atol=ATOL, err_msg=f"reward step {t}")
            if done.any():
                n_done += int(done.sum())
                np.testing.assert_allclose(info["terminal_observation"].cpu().numpy()[done], want_t[done], rtol=RTOL, atol=ATOL)
            if t % 5 == 4:
                assert np.array_equal(w.get_original_obs(), stacked), t          # raw stacks: bit-exact
                mean, var, sc = w._get_stats()
                np.testing.assert_allclose(mean, nz.obs_rms.mean, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"mean step {t}")
                np.testing.assert_allclose(var, nz.obs_rms.var, rtol=STAT_RTOL, atol=STAT_ATOL, err_msg=f"var step {t}")
                assert sc[0] == pytest.approx(nz.obs_rms.count, rel=COUNT_REL)
                assert sc[3] == pytest.approx(nz.ret_rms.count, rel=COUNT_REL)
                np.testing.assert_allclose([sc[1], sc[2]], [nz.ret_rms.mean, nz.ret_rms.var], rtol=STAT_RTOL)
                if snapshots is not None:
                    snapshots.append((mean, var, sc[0], sc[2]))
        assert n_done >= n                                                       # every environment finished at least once on average
        w.close()
    finally:
        if env_var:
            os.environ.pop(env_var, None)


def _forms_agree(snaps):
    """The three moment forms on the same batches: float64 rounding apart (tests/test_wrappers_gpu.py's bounds)."""
    ref = snaps["HLX_OBS_FULL_MOMENTS"]
    for form, got in snaps.items():
        assert len(got) == len(ref)
        for (m0, v0, c0, r0), (m1, v1, c1, r1) in zip(got, ref):
            assert c0 == c1 and abs(r0 - r1) <= 1e-13 * max(1.0, abs(r1)), form
            assert np.max(np.abs(m0 - m1)) <= 1e-12 * max(1.0, np.max(np.abs(m1))), form
            assert np.max(np.abs(v0 - v1)) <= 1e-11 * max(1.0, np.max(np.abs(v1))), form


PRESETS = {
    "medium/base": ("medium", "base", {}),
    "medium/v2dr": ("medium", "v2dr", {}),
    "medium/v2-los": ("medium", "v2", {"observation_mode": "los_frame"}),
    "medium/config-volley3": ("medium", "config", {"volley_mode": True, "volley_size": 3}),
}


@pytest.mark.parametrize("schedule", [2, 1, 0])
@pytest.mark.parametrize("preset", list(PRESETS))
def test_three_moment_forms_through_the_step(preset, schedule):
    n, T, seed = 300, 40, 17
    trace = _raw_trace(PRESETS[preset], n, T, seed, schedule)
    snaps = {}
    for form in (None, "HLX_OBS_NO_FUSE", "HLX_OBS_FULL_MOMENTS"):
        snaps[form] = []
        _wrapped_run(PRESETS[preset], n, T, seed, schedule, trace, env_var=form, snapshots=snaps[form])
    _forms_agree(snaps)


def test_noise_buffers_take_the_incremental_kernel():
    """Noise buffers set on the environment rule the fused form out (hlx_obs_step): the product's own route to
    hlx_obs_moments_inc_kernel; same statistics as the fused and the full forms of the Philox run."""
    n, T, seed, preset = 300, 40, 23, PRESETS["medium/v2dr"]
    trace = _raw_trace(preset, n, T, seed, None, noise=True)
    snaps = {"noise": []}
    _wrapped_run(preset, n, T, seed, None, trace, noise=True, snapshots=snaps["noise"])
    snaps["HLX_OBS_FULL_MOMENTS"] = []
    _wrapped_run(preset, n, T, seed, None, trace, env_var="HLX_OBS_FULL_MOMENTS", snapshots=snaps["HLX_OBS_FULL_MOMENTS"])
    _forms_agree(snaps)


# ----------------------------------------------------------------------------------------------------------------- C
@pytest.mark.parametrize("form", [None, "HLX_OBS_NO_FUSE"])
def test_wrappers_above_65536_environments(form):
    """n = 100 003: 1 563 step blocks (the fused finalize's tail loop and > 256 done masks per thread), moments kernels at
    1 024 blocks of ~98 environments, and the automatic load schedule 1."""
    n, T, seed, preset = 100003, 30, 29, PRESETS["medium/base"]
    probe = _make_env(preset, n, seed, None)
    assert probe.load_schedule == 1
    probe.close()
    trace = _raw_trace(preset, n, T, seed, None)
    _wrapped_run(preset, n, T, seed, None, trace, env_var=form)


def _frame(torch, step, rows, D, dev):
    """Frame of push `step` for environments `rows` (int64 device tensor): exact float32 values from a formula."""
    f = torch.arange(D, device=dev, dtype=torch.int32)
    v = (step * 7919 + rows.to(torch.int32)[:, None] * 131 + f[None, :] * 17) % 65521     # < 2^31 for n <= 2^20
    return (v.to(torch.float32) * 0.25 - 1000.0).contiguous()


def _done(torch, step, rows, n):
    d = ((rows * 40503 + step * 97) % 23) == 0
    if step == 3:
        d |= rows >= n - 5                  # the last rows of the batch
    return d


@pytest.mark.parametrize("n", [1048575, 1048576])
def test_rows_emit_on_both_sides_of_the_4_GiB_store_boundary(n):
    """hlx_obs_emit_rows_kernel writes the stacked batch through buffer stores while it is below 4 GiB and with plain stores at
    4 GiB (out_bytes = 0).  D 256, n_stack 4, norm_obs 0: n = 1 048 575 gives 4 294 963 200 bytes, n = 1 048 576 exactly 2^32.
    Peak device memory about 13 GiB (frame ring 4 GiB, output 4 GiB, one frame 1 GiB, comparison chunks)."""
    import torch
    D, S = 256, 4
    dev = torch.device("cuda", 0)
    pipe = _Pipe(n, D, S, training=False, norm_obs=False, norm_reward=False, outputs=False)
    try:
        rows_all = torch.arange(n, device=dev, dtype=torch.int64)
        age = torch.zeros(n, dtype=torch.int64, device=dev)
        fr = _frame(torch, 0, rows_all, D, dev)
        pipe.push_reset(fr)
        del fr
        for step in range(6):
            if step > 0:
                done = _done(torch, step, rows_all, n)
                fr = _frame(torch, step, rows_all, D, dev)
                term = done.to(torch.uint8)
                pipe.push(fr, term, None, None, None, term_out=False, rew_out=False)
                del fr
                age = torch.where(done, torch.zeros_like(age), torch.clamp(age + 1, max=S - 1))
                assert bool(done[-5:].all()) or step != 3
            # the stack, rebuilt chunk by chunk: position j (0 = oldest) holds the frame of push step - (S - 1 - j) where the
            # episode is that old, else zeros
            bad = 0
            for r0 in range(0, n, 1 << 17):
                rows = rows_all[r0:r0 + (1 << 17)]
                a = age[r0:r0 + (1 << 17)]
                want = torch.zeros((rows.numel(), S * D), dtype=torch.float32, device=dev)
                for j in range(S):
                    back = S - 1 - j
                    if step - back < 0:
                        continue
                    fb = _frame(torch, step - back, rows, D, dev)
                    want[:, j * D:(j + 1) * D] = torch.where((a >= back)[:, None], fb, torch.zeros_like(fb))
                bad += int((pipe.out[r0:r0 + rows.numel()] != want).sum())
            assert bad == 0, f"push {step}: {bad} elements differ"
    finally:
        pipe.close()


# ----------------------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize("D,S", [(7, 3), (26, 4)])
def test_two_fresh_pipelines_give_identical_bits(D, S):
    """Fixed-order, atomic-free reductions: the same push sequence twice -> the same outputs and statistics, bit for bit
    (scalar moments kernel; pair + incremental kernels)."""
    a, b = [], []
    _run_case(1000, D, S, seed=3, record=a)
    _run_case(1000, D, S, seed=3, record=b)
    assert len(a) == len(b) > 10
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


def test_fused_wrapper_form_is_deterministic():
    import torch
    from hlynr_intercept_amd.wrappers import VecFrameStack, VecNormalize
    n, T = 4099, 30
    runs = []
    for _ in range(2):
        w = VecNormalize(VecFrameStack(_make_env(PRESETS["medium/base"], n, 31, None), n_stack=4), norm_reward=True)
        g = torch.Generator(device=w.device).manual_seed(8)
        acts = torch.rand((T, n, 6), generator=g, device=w.device) * 2 - 1
        outs = [w.reset_torch().cpu().numpy().copy()]
        for t in range(T):
            o, r, _, _, _ = w.step_torch(acts[t])
            outs.append(o.cpu().numpy().copy())
            outs.append(r.cpu().numpy().copy())
        mean, var, sc = w._get_stats()
        outs += [mean, var, np.array(sc)]
        runs.append(outs)
        w.close()
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def _conditioning(D, S, top):
    import torch
    from oracle.vec_wrappers import FrameStack, Normalize
    n, T = 1000, 8
    ratios = np.array([1.0, 1e2, 1e3, top, 1.0][:D])
    rng = np.random.default_rng(11)
    std = np.array([0.5, 3.0, 1e-2, 2.0, 7.0][:D])
    dev = torch.device("cuda", 0)
    pipe = _Pipe(n, D, S, norm_reward=False, clip_obs=10.0, gamma=0.99, epsilon=1e-8)
    fs, nz = FrameStack(n, D, S), Normalize(n, D * S, norm_reward=False, clip_obs=10.0, gamma=0.99, epsilon=1e-8)
    try:
        def frame():
            return (ratios * std + std * rng.standard_normal((n, D))).astype(np.float32)
        f = frame()
        pipe.push_reset(torch.from_numpy(f).to(dev))
        nz.reset(fs.reset(f))
        _check_stats(pipe, nz, "reset")
        for t in range(T):
            f = frame()
            done = rng.random(n) < 0.1
            rw = rng.standard_normal(n).astype(np.float32)
            pipe.push(torch.from_numpy(f).to(dev), torch.from_numpy(done.astype(np.uint8)).to(dev), None, None,
                      torch.from_numpy(rw).to(dev), term_out=False)
            stacked, _ = fs.step(f, done, np.zeros((n, D), np.float32))
            want, _, _ = nz.step(stacked, rw, done, np.zeros_like(stacked))
            np.testing.assert_allclose(pipe.out.cpu().numpy(), want, rtol=RTOL, atol=ATOL)
            _check_stats(pipe, nz, f"push {t}")
    finally:
        pipe.close()


@pytest.mark.parametrize("D,S", [(4, 2), (5, 1)])
def test_one_pass_batch_variance_is_well_conditioned(D, S):
    """The batch variance is one-pass (sum(x^2)/n - mean^2, float64) where SB3 takes np.var (two-pass).  Columns with |mean|/std
    of 1, 1e2 and 1e3 agree with the float64 two-pass oracle at the bounds above (scalar kernel; pair + incremental kernels)."""
    _conditioning(D, S, 1.0)


@pytest.mark.xfail(strict=True, reason="known: at |mean|/std = 1e4 the one-pass batch variance is 2e-9..5e-9 away from the "
                   "two-pass oracle (include/hlx_obs.h, 'Conditioning')")
@pytest.mark.parametrize("D,S", [(4, 2), (5, 1)])
def test_one_pass_batch_variance_at_mean_over_std_1e4(D, S):
    _conditioning(D, S, 1e4)
