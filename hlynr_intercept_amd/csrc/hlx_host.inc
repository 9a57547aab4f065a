// hlx_host.inc -- host side of the C ABI declared in include/hlx.h (included by hlx_kernels.hip).
//
// Owns the state arena, evaluates the curriculum schedules, picks the kernel variant and issues
// the launches.  Nothing here touches Python or torch; every entry point returns an hlx_status.
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#ifdef HLX_AB_MINIMAL   // A/B experiment builds: 1 = the base variant only, 2 = the v2dr variant only
#undef HLX_BAKED_LIST
#if HLX_AB_MINIMAL == 2
#define HLX_BAKED_LIST(X) X(2, 0xc27fu)
#define HLX_AB_SPEC SPEC_V2DR
#else
#define HLX_BAKED_LIST(X) X(1, 0xc260u)
#define HLX_AB_SPEC SPEC_BASE
#endif
#endif

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(HLX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// kernel variants with the feature flags folded at compile time
constexpr uint32_t SPEC_BASE = HLX_F_VALIDATION | HLX_F_EVASION | HLX_F_GROUND;   // BASELINE.json config 2
constexpr uint32_t SPEC_V2 = SPEC_BASE | HLX_F_ATMOSPHERE | HLX_F_MACH_DRAG | HLX_F_ENH_WIND | HLX_F_THRUST_LAG;
constexpr uint32_t SPEC_V2DR = SPEC_V2 | HLX_F_DOMAIN_RAND;                       // BASELINE.json config 3
constexpr uint32_t SPEC_CONFIG = SPEC_BASE | HLX_F_ATMOSPHERE;                    // the reference's own config.yaml physics (ISA atmosphere only), medium / hard
constexpr uint32_t SPEC_CONFIG_EASY = SPEC_CONFIG & ~(uint32_t)HLX_F_EVASION;     // ... with the easy scenario (no missile evasion): BASELINE config 1
constexpr uint32_t SPEC_CONFIG_VOLLEY = SPEC_CONFIG | HLX_F_VOLLEY;               // ... in volley mode (inference.py --volley, BASELINE config 5)
enum { VAR_BASE = 0, VAR_V2, VAR_V2DR, VAR_CONFIG, VAR_CONFIG_EASY, VAR_CONFIG_VOLLEY, VAR_GENERIC, VAR_GENERIC_VOLLEY };
const char* const kVariantNames[] = {"base", "v2", "v2dr", "config", "config-easy", "config-volley", "generic", "generic-volley"};

}  // namespace

struct hlx_env {
    hlx_config cfg;
    KParams p;             // host copy of the device-resident parameter block
    KParams* p_dev;
    bool cur_valid, cos_valid;   // eval_curriculum has run / the cosine threshold belongs to half_beam
    KCfg& k = p.hot.c;
    int32_t n, device;
    uint64_t seed;
    int64_t env_offset;
    float4 *arena, *gring, *oring;
    int32_t* done_cnt;       // [2] in force: the library's own pair, or the caller's (hlx_set_done_counter)
    int32_t* done_cnt_own;
    unsigned long long* stamps;   // diagnostic builds only
    unsigned long long t;  // vec-step clock: RNG counter and delay-ring phase
    int variant;
    bool global_step_set;
    int64_t global_step;
    double cur[5];
    float radius, on_rel, g_rel;   // the curriculum scalars in force: kernel ARGUMENTS of every launch (no upload when they move)
    float cos_half_beam;           // the beam test's threshold on the cosine, re-derived when the half beam angle moves (hlx_kcfg.h)
    double half_beam;
    const double *step_noise, *reset_noise;
    bool prof;
    int64_t prof_launches;
    int32_t rollout_chunk;   // hlx_rollout: steps per launch (1 = one launch per step)
    float* rollout_terminal; // hlx_set_rollout_outputs: the optional hlx_step outputs that one-launch-per-step rollouts pass to every launch
    int32_t* rollout_done_idx;
    hlx_info_soa rollout_info;
    bool rollout_has_info;
    int baked;               // 1 + index of the baked constant table this configuration equals (hlx_baked_gen.h), 0 = none
    int32_t load_sched;      // 0: every load at kernel entry; 1: Kalman / ring loads as a second batch (<= two waves per SIMD);
                             // 2: that, plus the whole register file and the pool entry of a finished lane requested early (one wave per SIMD)
    double* pipe_partial;    // set by hlx_obs_step around ONE step launch (hlx_obs.inc): see KOpt::pipe_*
    double* pipe_returns;
    double pipe_gamma;
    int32_t pipe_stride, pipe_col0;
    uint32_t reset_epoch;    // hlx_reset calls at clock value `epoch_t` (16 bits): keys the spawn draws of explicit resets, so that
    unsigned long long epoch_t;   // two resets with no step between them do not replay the same episodes (hlx.h)
    // next-episode pool (hlx_kernels.hip): device arrays behind the rings in the arena allocation
    float4* pool;
    uint32_t *pool_tag, *ep_cur;
    int32_t* rf_cnt;         // [2]: respawns computed inside a step launch for want of an entry (misses); [3]: ... in a crowded wave
    bool pool_on;            // step launches look their next episode up in the pool
    bool pool_dirty;         // every entry is stale (explicit reset, new seed, curriculum scalars, injected state): fill all before the next step
    bool ep_zero_pending;    // hlx_set_seed: the per-environment episode counters restart with the next launch
    int32_t pool_since, pool_interval;   // steps since the last fill; fill every `pool_interval` steps
    bool pool_suspended;     // a sensor reliability moved less than HLX_POOL_QUIET_STEPS step launches ago: entries are not used
    int32_t pool_quiet;      // step launches since a reliability last moved
    int64_t pool_full_fills, pool_partial_fills, pool_suspended_steps;   // diagnostics (hlx_get_episode_pool_stats)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used;
};

namespace {

void eval_curriculum(hlx_env* e) {
    const hlx_config& c = e->cfg;
    const double gs = e->global_step_set ? (double)e->global_step : 0.0;
    double radius = c.final_radius;                                         // environment.py:223-234
    if (c.flags & HLX_F_USE_CURRICULUM) {
        double progress = std::fmin(1.0, gs / c.curriculum_steps);
        radius = c.initial_radius * (1.0 - progress) + c.final_radius * progress;
    }
    double beam = c.radar_beam_width, on_rel = 1.0, g_rel = 1.0, noise = 0.05;  // core.py:286-288
    if (c.flags & HLX_F_RADAR_CURRICULUM) {
        auto lerp = [&](const double s[4]) {                                // environment.py:296-345
            if (!e->global_step_set) return s[0];                           // constructor state :153-185
            if (gs < s[2]) return s[0];
            if (gs >= s[3]) return s[1];
            double p = (gs - s[2]) / (s[3] - s[2]);
            return s[0] * (1.0 - p) + s[1] * p;
        };
        beam = lerp(c.rc_beam); on_rel = lerp(c.rc_onboard); g_rel = lerp(c.rc_ground); noise = lerp(c.rc_noise);
    }
    e->cur[0] = radius; e->cur[1] = beam; e->cur[2] = on_rel; e->cur[3] = g_rel; e->cur[4] = noise;
    e->radius = (float)radius;
    const double hb = (beam / 2.0) * (M_PI / 180.0);                        // core.py:548 np.radians -> float64
    if (hb != e->half_beam || !e->cos_valid) { e->cos_half_beam = beam_cos_threshold(hb); e->cos_valid = true; }   // (31 acosf calls: only when it moved)
    e->half_beam = hb;
    // A first observation depends on the beam width and on the two reliabilities (not on the intercept radius).  The beam
    // width -- the one scalar the reference's shipped curriculum ramps, at every call of set_training_step_count -- needs
    // nothing here: every prepared episode carries the beam test it was computed with and is checked against the threshold in
    // force when it is used (hlx_kernels.hip, respawn block).  A reliability that moves makes every entry stale; while one is
    // MOVING the pool is suspended (finished environments compute their next episode in place: what the pool-less kernel does)
    // and it is filled again once the scalars have stood still for HLX_POOL_QUIET_STEPS step launches -- not ahead of every step
    // of a ramp, as in round 3 (a full fill is a 12-45 us launch in front of a 9 us step).
    if (e->cur_valid && ((float)on_rel != e->on_rel || (float)g_rel != e->g_rel)) { e->pool_suspended = true; e->pool_quiet = 0; }
    e->on_rel = (float)on_rel;
    e->g_rel = (float)g_rel;
    e->cur_valid = true;
}


double f4_as_d(float lo, float hi) { uint32_t a, b; memcpy(&a, &lo, 4); memcpy(&b, &hi, 4); uint64_t u = ((uint64_t)b << 32) | a; double d; memcpy(&d, &u, 8); return d; }
void d_as_f2(double d, float& lo, float& hi) { uint64_t u; memcpy(&u, &d, 8); uint32_t a = (uint32_t)u, b = (uint32_t)(u >> 32); memcpy(&lo, &a, 4); memcpy(&hi, &b, 4); }
// constructor values of the per-episode constants (G_MISC, G_THRUST.w) of every 64-env block
__global__ void hlx_init_misc_kernel(float4* arena, float4 v, float cd_super) {
    arena[((size_t)blockIdx.x * N_GROUPS + G_MISC) * 64 + threadIdx.x] = v;
    arena[((size_t)blockIdx.x * N_GROUPS + G_THRUST) * 64 + threadIdx.x] = make_float4(0.f, 0.f, 0.f, cd_super);
}

// Re-upload the optional-buffer block / the curriculum scalars only when they changed (enqueued on the launch
// stream, ahead of the launch that needs them; hipMemcpyAsync stages pageable memory at call time).
int sync_params(hlx_env* e, const KOpt& want, hipStream_t s) {
    if (memcmp(&want, &e->p.hot.opt, sizeof(KOpt)) != 0) {
        e->p.hot.opt = want;
        HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(e->p_dev) + offsetof(KParams, hot) + offsetof(KHot, opt), &e->p.hot.opt, sizeof(KOpt),
                               hipMemcpyHostToDevice, s));
    }
    return HLX_OK;
}

bool info_any(const hlx_info_soa& in) {
    return in.distance || in.min_distance || in.fuel || in.flags || in.episode_return || in.episode_length || in.missiles ||
           in.interceptor_pos || in.missile_pos || in.steps || in.missile_min_distances || in.radar_debug || in.fuel_used || in.packed;
}
// hlx_info_soa.packed replaces the nine standard planes: both at once would be written twice, by two code paths
const char* info_invalid(const hlx_env* e, const hlx_info_soa* in) {
    if (!in) return nullptr;
    if (in->radar_debug && !(e->cfg.flags & HLX_F_RADAR_DEBUG)) return "info.radar_debug needs an environment created with HLX_F_RADAR_DEBUG";
    if (in->packed && (in->distance || in->min_distance || in->fuel || in->fuel_used || in->flags || in->missiles || in->interceptor_pos ||
                       in->missile_pos || in->steps))
        return "info.packed carries the nine standard keys: their separate planes must be NULL";
    return nullptr;
}

uint32_t ring_slots(const hlx_env* e) {
    const unsigned long long g_cap = (unsigned long long)(e->k.g_delay + 1), o_cap = (unsigned long long)e->k.o_cap;
    // ground read slot (t - g_delay) mod cap == (t + 1) mod cap | ground write slot | onboard write slot
    const uint32_t g_planes = (e->cfg.flags & HLX_F_GROUND) ? (uint32_t)g_cap : 0u, o_planes = e->k.o_delay > 0 ? (uint32_t)o_cap : 0u;
    const hlx_info_soa& in = e->p.hot.opt.info;     // as uploaded by sync_params before this launch
    const bool any_info = info_any(in);
    const bool pipe = e->p.hot.opt.pipe_partial != nullptr;      // bit 22: the observation pipeline rides on this launch (hlx_obs_step)
    // bit 23: hlx_info_soa.packed is given (the contract form a VecEnv facade passes): the nine standard keys leave as three
    // 16-byte words per environment
    // bit 24: the next-episode pool is in use (the lone-wave load schedule only: hlx_kernels.hip)
    return (uint32_t)((e->t + 1ull) % g_cap) | ((uint32_t)(e->t % g_cap) << 4) | ((uint32_t)(e->t % o_cap) << 8) |
           (g_planes << 12) | (o_planes << 16) | (any_info ? 1u << 20 : 0u) | (pipe ? 1u << 22 : 0u) | (in.packed ? 1u << 23 : 0u) |
           ((e->pool_on && e->load_sched == 2 && !e->pool_suspended) ? 1u << 24 : 0u);
}

struct KIo {   // caller buffers of one launch
    const float* actions;
    float* obs;
    float* reward;
    uint8_t* term;
    uint8_t* trunc;
};

// Philox counter word of a launch: the vec-step clock (40 bits: the counter's fourth word is `(clock >> 32) << 8 | stream`,
// so 56 bits of this argument reach the generator); a reset-only launch (MODE 1) also carries the 16-bit reset epoch in bits
// 40-55 (the kernel uses its clock argument for the RNG only; ring slots and the done counter come from `slots` / MODE 0).
// The epoch counts the resets at the CURRENT clock value: it is 0 again once a step has advanced the clock.
uint32_t cur_epoch(const hlx_env* e) { return e->t == e->epoch_t ? (e->reset_epoch & 0xFFFFu) : 0u; }
template <int MODE>
unsigned long long clock_arg(const hlx_env* e) {
    return MODE == 1 ? ((e->t & 0xFFFFFFFFFFull) | ((unsigned long long)cur_epoch(e) << 40)) : e->t;
}

template <int MODE, bool NOISE>
hipError_t launch_v(const hlx_env* e, const KIo& io, hipStream_t s, uint32_t extra_slots = 0u) {
    dim3 grid((unsigned)((e->n + 63) / 64)), block(64);
    const KParams* P = e->p_dev;
    const uint32_t slots = ring_slots(e) | extra_slots;
    // the production step kernel exists in three load schedules (hlx_kernels.hip, LATE); parity / reset / pool-fill launches use the plain one
    const int sched = (MODE == 0 && !NOISE) ? e->load_sched : 0;
    constexpr int L1 = (MODE == 0 && !NOISE) ? 1 : 0, L2 = (MODE == 0 && !NOISE) ? 2 : 0;
#define HLX_LAUNCH_AS(SPEC, LATE_, BAKE_)                                                                         \
    hlx_launchers::hlx_launch<SPEC, MODE, NOISE, false, LATE_, BAKE_>(grid, s, hlx_launchers::StepArgs{e->arena, P, \
                       io.actions, clock_arg<MODE>(e), (unsigned long long)e->seed, (long long)e->env_offset, (int)e->n, slots, \
                       io.obs, io.reward, io.term, io.trunc, e->radius, e->cos_half_beam, e->on_rel, e->g_rel, 1, 0, 1})
#define HLX_LAUNCH(SPEC)                                                                                          \
    do {                                                                                                          \
        if (sched == 2) HLX_LAUNCH_AS(SPEC, L2, 0);                                                               \
        else if (sched == 1) HLX_LAUNCH_AS(SPEC, L1, 0);                                                          \
        else HLX_LAUNCH_AS(SPEC, 0, 0);                                                                           \
    } while (0)
    if (MODE == 0 && !NOISE && e->baked) {   // production step launch of a shipped preset: constants are literals
#define HLX_BAKED_CASE(ID, FLAGS)                                                                                 \
        case ID:                                                                                                  \
            if (sched == 2) HLX_LAUNCH_AS((FLAGS) & KF_CODEGEN_MASK, L2, ((MODE == 0 && !NOISE) ? ID : 0));       \
            else if (sched == 1) HLX_LAUNCH_AS((FLAGS) & KF_CODEGEN_MASK, L1, ((MODE == 0 && !NOISE) ? ID : 0));  \
            else HLX_LAUNCH_AS((FLAGS) & KF_CODEGEN_MASK, 0, ((MODE == 0 && !NOISE) ? ID : 0));                   \
            return hipGetLastError();
        switch (e->baked) { HLX_BAKED_LIST(HLX_BAKED_CASE) default: break; }
#undef HLX_BAKED_CASE
    }
    switch (e->variant) {
#ifndef HLX_AB_MINIMAL
        case VAR_BASE: HLX_LAUNCH(SPEC_BASE); break;
        case VAR_V2: HLX_LAUNCH(SPEC_V2); break;
        case VAR_V2DR: HLX_LAUNCH(SPEC_V2DR); break;
        case VAR_CONFIG: HLX_LAUNCH(SPEC_CONFIG); break;
        case VAR_CONFIG_EASY: HLX_LAUNCH(SPEC_CONFIG_EASY); break;
        case VAR_CONFIG_VOLLEY: HLX_LAUNCH(SPEC_CONFIG_VOLLEY); break;
        case VAR_GENERIC_VOLLEY: HLX_LAUNCH(KF_DYNAMIC | (uint32_t)HLX_F_VOLLEY); break;
        default: HLX_LAUNCH(KF_DYNAMIC); break;
#else   // A/B experiment builds (tools/ab_build.sh -DHLX_AB_MINIMAL): the base variant only, seconds instead of minutes to compile
        default: HLX_LAUNCH(HLX_AB_SPEC); break;
#endif
    }
#undef HLX_LAUNCH
#undef HLX_LAUNCH_AS
    return hipGetLastError();
}
// fused rollout: T steps in one launch (state resident in registers), outputs rotate over `out_slots` slots
hipError_t launch_fused(const hlx_env* e, const KIo& io, int T, int out_slot0, int out_slots, hipStream_t s) {
    dim3 grid((unsigned)((e->n + 63) / 64)), block(64);
    const KParams* P = e->p_dev;
    const uint32_t slots = ring_slots(e);
    if (e->baked) {
#define HLX_BAKED_CASE(ID, FLAGS)                                                                                 \
        case ID:                                                                                                  \
            hlx_launchers::hlx_launch<(FLAGS) & KF_CODEGEN_MASK, 0, false, true, 0, ID>(grid, s, hlx_launchers::StepArgs{e->arena, P, io.actions, \
                               e->t, (unsigned long long)e->seed, (long long)e->env_offset, (int)e->n, slots, io.obs, io.reward, io.term, \
                               io.trunc, e->radius, e->cos_half_beam, e->on_rel, e->g_rel, T, out_slot0, out_slots});                       \
            return hipGetLastError();
        switch (e->baked) { HLX_BAKED_LIST(HLX_BAKED_CASE) default: break; }
#undef HLX_BAKED_CASE
    }
#define HLX_LAUNCH(SPEC)                                                                                          \
    hlx_launchers::hlx_launch<SPEC, 0, false, true, 0, 0>(grid, s, hlx_launchers::StepArgs{e->arena, P, io.actions, e->t,  \
                       (unsigned long long)e->seed, (long long)e->env_offset, (int)e->n, slots, io.obs, io.reward, \
                       io.term, io.trunc, e->radius, e->cos_half_beam, e->on_rel, e->g_rel, T, out_slot0, out_slots})
    switch (e->variant) {
#ifndef HLX_AB_MINIMAL
        case VAR_BASE: HLX_LAUNCH(SPEC_BASE); break;
        case VAR_V2: HLX_LAUNCH(SPEC_V2); break;
        case VAR_V2DR: HLX_LAUNCH(SPEC_V2DR); break;
        case VAR_CONFIG: HLX_LAUNCH(SPEC_CONFIG); break;
        case VAR_CONFIG_EASY: HLX_LAUNCH(SPEC_CONFIG_EASY); break;
        case VAR_CONFIG_VOLLEY: HLX_LAUNCH(SPEC_CONFIG_VOLLEY); break;
        case VAR_GENERIC_VOLLEY: HLX_LAUNCH(KF_DYNAMIC | (uint32_t)HLX_F_VOLLEY); break;
        default: HLX_LAUNCH(KF_DYNAMIC); break;
#else   // A/B experiment builds (tools/ab_build.sh -DHLX_AB_MINIMAL): the base variant only, seconds instead of minutes to compile
        default: HLX_LAUNCH(HLX_AB_SPEC); break;
#endif
    }
#undef HLX_LAUNCH
    return hipGetLastError();
}
template <int MODE>
hipError_t launch(const hlx_env* e, const KIo& io, hipStream_t s) {
    // parity mode (draws injected through hlx_set_noise) runs the NOISE instantiation of the same source
    return (e->step_noise || e->reset_noise) ? launch_v<MODE, true>(e, io, s) : launch_v<MODE, false>(e, io, s);
}

// Next-episode pool: one MODE-2 launch prepares the next episode of every environment (`all`: after an explicit reset, a new
// seed, moved curriculum scalars, injected state) or of the environments the steps since the last fill have listed.  Enqueued
// on the stream of the step launches around it.
int pool_fill(hlx_env* e, bool all, hipStream_t s) {
    if (e->ep_zero_pending) {
        HIP_TRY(hipMemsetAsync(e->ep_cur, 0, sizeof(uint32_t) * (((size_t)e->n + 63) / 64) * 64, s));
        e->ep_zero_pending = false;
        all = true;
    }
    KIo io{nullptr, nullptr, nullptr, nullptr, nullptr};
    HIP_TRY((launch_v<2, false>(e, io, s, all ? 0u : 1u << 25)));
    (all ? e->pool_full_fills : e->pool_partial_fills) += 1;
    if (all) e->pool_dirty = false;     // (the blocks' used-entry masks keep what they hold: the next fill finds those entries renewed and skips them)
    e->pool_since = 0;
    return HLX_OK;
}
// Ahead of a step launch: a stale pool is filled entirely; the entries used since the last fill are renewed once `pool_interval`
// steps have gone by -- ahead of launches that can use them only (`consumes`: the step launches without noise buffers, every one of
// them two-pass under the lone-wave schedule; the fused rollout computes its respawns in place, and a rollout made of it alone never
// pays for a fill).
int pool_before_step(hlx_env* e, hipStream_t s, bool consumes = false) {
    if (e->ep_zero_pending && (!e->pool_on || e->load_sched != 2)) {
        HIP_TRY(hipMemsetAsync(e->ep_cur, 0, sizeof(uint32_t) * (((size_t)e->n + 63) / 64) * 64, s));
        e->ep_zero_pending = false;
    }
    if (!e->pool_on || e->load_sched != 2) return HLX_OK;     // (the pool serves the lone-wave schedule only)
    if (e->ep_zero_pending) return pool_fill(e, true, s);
    if (!consumes) return HLX_OK;
    if (e->pool_suspended) {       // a sensor reliability has been moving: wait until it has stood still, then renew everything
        e->pool_suspended_steps += 1;
        if (++e->pool_quiet < HLX_POOL_QUIET_STEPS) return HLX_OK;
        e->pool_suspended = false;
        e->pool_dirty = true;
        // (this launch was given its `slots` word AFTER this call: it already uses the entries the fill below prepares)
    }
    if (e->pool_dirty) return pool_fill(e, true, s);
    if (e->pool_since >= e->pool_interval) return pool_fill(e, false, s);
    return HLX_OK;
}

int prof_event(hlx_env* e, hipStream_t s) {
    if (e->ev_used == e->ev_pool.size()) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        e->ev_pool.push_back(ev);
    }
    HIP_TRY(hipEventRecord(e->ev_pool[e->ev_used++], s));
    return HLX_OK;
}

// Philox draws of the next step -> slot-major arrays (same device functions as the fused kernel)
__global__ __launch_bounds__(64) void hlx_fill_noise_kernel(double* sn, double* rn, int n, unsigned long long t,
                                                            uint32_t seed_lo, uint32_t seed_hi, long long env_offset,
                                                            const uint32_t* ep_cur /* NULL: reset draws keyed by the clock word */) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const size_t N = (size_t)n;
    const unsigned long long gid = (unsigned long long)(env_offset + i);
    Rng rng{uint2{seed_lo, seed_hi}, (uint32_t)gid, (uint32_t)(gid >> 32), (uint32_t)t, (uint32_t)(t >> 32)};
    float z[4];
    if (sn) {
        double* S = sn + i;
        float m[12];
        rng.normals4(RS_STEP_N0, m[0], m[1], m[2], m[3]);
        rng.normals4(RS_STEP_N1, m[4], m[5], m[6], m[7]);
        rng.normals4(RS_STEP_N2, m[8], m[9], m[10], m[11]);
        S[0] = m[0]; S[N] = m[1]; S[2 * N] = m[2];                     // evasion
        S[3 * N] = m[3]; S[4 * N] = m[4]; S[5 * N] = m[5];             // wind
        S[13 * N] = m[6]; S[14 * N] = m[7]; S[15 * N] = m[8];          // ground pos
        S[16 * N] = m[9]; S[17 * N] = m[10]; S[18 * N] = m[11];        // ground vel
        uint4 x = rng.raw(RS_STEP_U);
        S[11 * N] = u01(x.x); S[12 * N] = u01(x.y); S[19 * N] = u01(x.z); S[6 * N] = u01(x.w);
        V3 g; float e;
        gust_draws(rng, g, e);
        S[7 * N] = g.x; S[8 * N] = g.y; S[9 * N] = g.z; S[10 * N] = e;
        for (int k = 1; k < HLX_MAX_VOLLEY; ++k) {                     // volley missiles 1..3: evasion
            rng.normals4(RS_STEP_V1 + (uint32_t)(k - 1), z[0], z[1], z[2], z[3]);
            S[(20 + 3 * (k - 1)) * N] = z[0]; S[(21 + 3 * (k - 1)) * N] = z[1]; S[(22 + 3 * (k - 1)) * N] = z[2];
        }
        for (int k = 29; k < HLX_STEP_SLOTS; ++k) S[k * N] = 0.0;
    }
    if (rn) {
        double* R = rn + i;
        // the draws of an auto-reset are keyed by the index of the episode that starts (hlx_kernels.hip), those of an explicit
        // reset by the clock word
        if (ep_cur) rng = Rng{rng.key, rng.id_lo, rng.id_hi, ep_cur[i] + 1u, 0xFFFFFFu};
        uint4 x0 = rng.raw(RS_RESET_U0), x1 = rng.raw(RS_RESET_U1), x2 = rng.raw(RS_RESET_U2);
        R[0] = u01(x0.x); R[N] = u01(x0.y); R[2 * N] = u01(x0.z); R[3 * N] = u01(x0.w);
        R[4 * N] = u01(x1.x); R[5 * N] = u01(x1.y); R[6 * N] = u01(x1.z); R[7 * N] = u01(x1.w);
        R[8 * N] = u01(x2.x); R[9 * N] = u01(x2.y);
        uint4 xo = rng.raw(RS_RESET_OBS_U);
        R[10 * N] = u01(xo.x); R[11 * N] = u01(xo.y); R[18 * N] = u01(xo.z);
        rng.normals4(RS_RESET_GPOS, z[0], z[1], z[2], z[3]); R[12 * N] = z[0]; R[13 * N] = z[1]; R[14 * N] = z[2];
        rng.normals4(RS_RESET_GVEL, z[0], z[1], z[2], z[3]); R[15 * N] = z[0]; R[16 * N] = z[1]; R[17 * N] = z[2];
        rng.normals4(RS_DR0, z[0], z[1], z[2], z[3]); R[19 * N] = z[0]; R[20 * N] = z[1]; R[21 * N] = z[2]; R[22 * N] = z[3];
        rng.normals4(RS_DR1, z[0], z[1], z[2], z[3]); R[23 * N] = z[0]; R[24 * N] = z[1]; R[25 * N] = z[2]; R[26 * N] = z[3];
        rng.normals4(RS_DR2, z[0], z[1], z[2], z[3]); R[27 * N] = z[0]; R[28 * N] = z[1]; R[29 * N] = z[2]; R[30 * N] = z[3];
        rng.normals4(RS_DR3, z[0], z[1], z[2], z[3]); R[31 * N] = z[0];
        for (int k = 1; k < HLX_MAX_VOLLEY; ++k) {                     // volley missiles 1..3: spawn uniforms
            const uint4 x = rng.raw(RS_RESET_V1 + (uint32_t)(k - 1));
            double* B = R + (size_t)(32 + 4 * (k - 1)) * N;
            B[0] = u01(x.x); B[N] = u01(x.y); B[2 * N] = u01(x.z); B[3 * N] = u01(x.w);
        }
        for (int k = 44; k < HLX_RESET_SLOTS; ++k) R[k * N] = 0.0;
    }
}

// hlx_selftest_math: the device copies of the restated transcendentals, evaluated element-wise (tests compare them bit
// for bit with oracle/ref_math.h, which tests/test_ref_math.py pins against libm / numpy)
__global__ void hlx_selftest_math_kernel(int kind, const float* x, float y, float* out, long long n) {
    static_assert(sizeof(PowTab) == 512, "the step kernel stages the table with one 8-byte word per lane");
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 2) {          // sqrt_rn against the compiler's correctly rounded sqrtf: 1.0 where the bits agree
        out[i] = __float_as_uint(sqrt_rn(x[i])) == __float_as_uint(__builtin_sqrtf(x[i])) ? 1.0f : 0.0f;
    } else if (kind == 3) {   // dsqrt_pos against the compiler's sqrt on float64 arguments |x * y| + x * x (sums of products, >= 0)
        const double a = fabs((double)x[i] * (double)y) + (double)x[i] * (double)x[i];
        out[i] = __double_as_longlong(dsqrt_pos(a)) == __double_as_longlong(sqrt(a)) ? 1.0f : 0.0f;
    } else
        out[i] = kind == 0 ? pow_ref(x[i], y, &HLX_POW_TAB) : exp_np(x[i]);
}

}  // namespace

extern "C" {

int hlx_selftest_math(int32_t kind, const float* x, float y, float* out, int64_t n, void* stream) {
    if (kind < 0 || kind > 3 || !x || !out || n < 0) return fail(HLX_ERR_INVALID, "hlx_selftest_math: bad argument");
    if (n == 0) return HLX_OK;
    hipLaunchKernelGGL(hlx_selftest_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)kind, x, y,
                       out, (long long)n);
    HIP_TRY(hipGetLastError());
    return HLX_OK;
}

const char* hlx_last_error(void) { return g_err.c_str(); }
const char* hlx_version(void) { return "hlx 0.1 (gfx950)"; }
int32_t hlx_sizeof_config(void) { return (int32_t)sizeof(hlx_config); }
int32_t hlx_sizeof_env_state(void) { return (int32_t)sizeof(hlx_env_state); }
int32_t hlx_sizeof_info_soa(void) { return (int32_t)sizeof(hlx_info_soa); }
int32_t hlx_abi_version(void) { return HLX_ABI_VERSION; }
#ifndef HLX_HOT_FROM_MEMORY
#define HLX_HOT_FROM_MEMORY 0
#endif
int32_t hlx_hot_words_from_memory(void) { return HLX_HOT_FROM_MEMORY; }
int32_t hlx_num_envs(const hlx_env* e) { return e ? e->n : 0; }
int64_t hlx_vec_steps(const hlx_env* e) { return e ? (int64_t)e->t : 0; }
const char* hlx_kernel_variant(const hlx_env* e) { return e ? kVariantNames[e->variant] : ""; }
const char* hlx_kernel_baked(const hlx_env* e) { return (e && e->baked) ? HLX_BAKED_NAME[e->baked - 1] : ""; }

int hlx_create(const hlx_config* cfg, int32_t n_envs, int32_t device, uint64_t seed, int64_t env_id_offset,
               hlx_env** out) {
    if (!cfg || !out) return fail(HLX_ERR_INVALID, "hlx_create: null argument");
    *out = nullptr;
    if (n_envs <= 0) return fail(HLX_ERR_INVALID, "hlx_create: n_envs must be > 0 (got %d)", n_envs);
    if (cfg->max_steps <= 0 || cfg->max_steps > HLX_MAX_STEPS)
        return fail(HLX_ERR_INVALID, "hlx_create: max_steps %d outside [1, %d]", cfg->max_steps, HLX_MAX_STEPS);
    if ((cfg->flags & HLX_F_VOLLEY) && (cfg->volley_size < 1 || cfg->volley_size > HLX_MAX_VOLLEY))
        return fail(HLX_ERR_INVALID, "hlx_create: volley_size %d outside [1, %d]", cfg->volley_size, HLX_MAX_VOLLEY);
    if (!(cfg->dt > 0.0)) return fail(HLX_ERR_INVALID, "hlx_create: dt must be > 0");
    if (cfg->onboard_delay < 0 || cfg->onboard_delay > HLX_MAX_DELAY || cfg->ground_delay < 0 ||
        cfg->ground_delay > HLX_MAX_DELAY)
        return fail(HLX_ERR_INVALID, "hlx_create: sensor delays must be within [0, %d] samples", HLX_MAX_DELAY);
    if ((cfg->flags & HLX_F_OBS_BODY) && (cfg->flags & HLX_F_OBS_LOS))
        return fail(HLX_ERR_INVALID, "hlx_create: observation mode flags are mutually exclusive");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(HLX_ERR_INVALID, "hlx_create: device %d not in [0, %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hlx_env* e = new (std::nothrow) hlx_env();
    if (!e) return fail(HLX_ERR_NOMEM, "hlx_create: out of host memory");
    e->cfg = *cfg;
    memset(&e->p, 0, sizeof e->p);
    build_kcfg(*cfg, e->p.hot.c, e->p.cold);
    e->p_dev = nullptr; e->cur_valid = false; e->cos_valid = false; e->half_beam = 0.0;
    e->n = n_envs; e->device = device; e->seed = seed; e->env_offset = env_id_offset;
    e->t = 0; e->global_step_set = false; e->global_step = 0;
    e->step_noise = e->reset_noise = nullptr;
    e->prof = false; e->ev_used = 0; e->prof_launches = 0; e->rollout_chunk = 1; e->reset_epoch = 0; e->epoch_t = 0;
    e->pipe_partial = e->pipe_returns = nullptr; e->pipe_gamma = 0.0; e->pipe_stride = e->pipe_col0 = 0;
    e->rollout_terminal = nullptr; e->rollout_done_idx = nullptr; e->rollout_has_info = false; memset(&e->rollout_info, 0, sizeof e->rollout_info);
    e->arena = e->gring = e->oring = nullptr; e->done_cnt = e->done_cnt_own = nullptr; e->stamps = nullptr;
    e->pool = nullptr; e->pool_tag = e->ep_cur = nullptr; e->rf_cnt = nullptr;
    e->pool_on = getenv("HLX_NO_POOL") == nullptr;       // (diagnostic switch for A/B runs; hlx_set_episode_pool is the API)
    e->pool_dirty = true; e->ep_zero_pending = false; e->pool_since = 0; e->pool_interval = HLX_POOL_INTERVAL_DEFAULT;
    e->pool_suspended = false; e->pool_quiet = 0; e->pool_full_fills = e->pool_partial_fills = e->pool_suspended_steps = 0;
    if (const char* ov = getenv("HLX_POOL_INTERVAL")) { const int v = atoi(ov); if (v > 0) e->pool_interval = v; }
    const uint32_t cg = cfg->flags & KF_CODEGEN_MASK;
    e->variant = (cg == SPEC_BASE) ? VAR_BASE : (cg == SPEC_V2) ? VAR_V2 : (cg == SPEC_V2DR) ? VAR_V2DR : (cg == SPEC_CONFIG) ? VAR_CONFIG
                 : (cg == SPEC_CONFIG_EASY) ? VAR_CONFIG_EASY : (cg == SPEC_CONFIG_VOLLEY) ? VAR_CONFIG_VOLLEY
                 : (cg & HLX_F_VOLLEY) ? VAR_GENERIC_VOLLEY : VAR_GENERIC;
    e->baked = 0;
    static_assert(sizeof(KCfg) == 4 * HLX_BAKED_DWORDS && sizeof(KCold) == 4 * HLX_BAKED_COLD_DWORDS, "hlx_baked_gen.h is stale: rebuild through hlynr_intercept_amd/build.py");
    if (!getenv("HLX_NO_BAKED"))     // (diagnostic switch for A/B runs)
        for (int i = 0; i < HLX_BAKED_COUNT; ++i)
            if (memcmp(&e->p.hot.c, HLX_BAKED_TAB[i], sizeof(KCfg)) == 0 && memcmp(&e->p.cold, HLX_BAKED_COLD[i], sizeof(KCold)) == 0) { e->baked = i + 1; break; }
    eval_curriculum(e);
    {   // second-batch loads pay while the load phase is exposed: up to two 64-env waves per SIMD
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
        const int blocks = (n_envs + 63) / 64;
        e->load_sched = blocks <= 4 * cus ? 2 : blocks <= 8 * cus ? 1 : 0;
        if (const char* ov = getenv("HLX_LATE_LOADS")) if (ov[0] >= '0' && ov[0] <= '2') e->load_sched = ov[0] - '0';   // diagnostic override; see hlx_set_load_schedule
    }
    const size_t N = (size_t)n_envs;
    // a ground station always gets at least one ring slot so that the kernel's entry loads need no guard
    const size_t g_planes = (size_t)((cfg->flags & HLX_F_GROUND) ? (e->k.g_delay + 1) * GROUND_RING_WORDS16 : 0);
    const size_t o_planes = (size_t)(e->k.o_delay > 0 ? e->k.o_cap : 0);
    const size_t NB = ((N + 63) / 64) * 64;   // arena rows padded to whole 64-env blocks
    // state groups | ground ring | onboard ring | next-episode pool and its bookkeeping (hlx_kargs.h pool_aux_words16)
    const size_t arena_words16 = NB * N_GROUPS + N * (g_planes + o_planes), total_words16 = arena_words16 + pool_aux_words16(NB / 64);
    hipError_t err = hipMalloc(&e->arena, sizeof(float4) * total_words16);
    if (err == hipSuccess) { err = hipMalloc(&e->done_cnt_own, 2 * sizeof(int32_t)); e->done_cnt = e->done_cnt_own; }
#ifdef HLX_STAMPS
    if (err == hipSuccess) err = hipMalloc(&e->stamps, sizeof(unsigned long long) * 16 * ((N + 63) / 64));
#endif
    if (err == hipSuccess) err = hipMalloc(&e->p_dev, sizeof(KParams));
    if (err != hipSuccess) {
        int rc = fail(err == hipErrorOutOfMemory ? HLX_ERR_NOMEM : HLX_ERR_HIP, "hlx_create: hipMalloc: %s",
                      hipGetErrorString(err));
        hlx_destroy(e);
        return rc;
    }
    e->gring = e->arena + NB * N_GROUPS;
    e->oring = e->gring + N * g_planes;
    e->pool = e->arena + arena_words16;                                  // the kernel derives the same addresses from (arena, n, slots)
    e->pool_tag = reinterpret_cast<uint32_t*>(e->pool + NB * POOL_GROUPS);
    e->ep_cur = e->pool_tag + NB;
    e->rf_cnt = reinterpret_cast<int32_t*>(e->ep_cur + NB);
    e->p.gring = e->gring; e->p.oring = e->oring; e->p.n = n_envs;
    e->p.done_cnt = e->done_cnt;
    e->p.stamps = e->stamps;
    e->p.seed_lo = (uint32_t)seed; e->p.seed_hi = (uint32_t)(seed >> 32); e->p.env_offset = env_id_offset;
    err = hipMemcpy(e->p_dev, &e->p, sizeof(KParams), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        int rc = fail(HLX_ERR_HIP, "hlx_create: parameter upload: %s", hipGetErrorString(err));
        hlx_destroy(e);
        return rc;
    }
    // constructor state: everything zero except the constants domain randomisation perturbs
    err = hipMemset(e->arena, 0, sizeof(float4) * total_words16);
    if (err == hipSuccess) {
        float4 misc0;
        d_as_f2(288.15, misc0.x, misc0.y);
        misc0.z = 0.3f; misc0.w = (float)(cfg->transonic_peak_multiplier - 1.0);
        hlx_init_misc_kernel<<<dim3((unsigned)(NB / 64)), dim3(64), 0, nullptr>>>(
            e->arena, misc0, (float)(0.3 * cfg->supersonic_multiplier));
        err = hipGetLastError();
        if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
    }
    if (err == hipSuccess) err = hipMemset(e->done_cnt, 0, 2 * sizeof(int32_t));
    if (err != hipSuccess) {
        int rc = fail(HLX_ERR_HIP, "hlx_create: arena initialisation: %s", hipGetErrorString(err));
        hlx_destroy(e);
        return rc;
    }
    *out = e;
    return HLX_OK;
}

int hlx_destroy(hlx_env* e) {
    if (!e) return HLX_OK;
    hipSetDevice(e->device);
    for (hipEvent_t ev : e->ev_pool) hipEventDestroy(ev);
    if (e->arena) hipFree(e->arena);
    if (e->done_cnt_own) hipFree(e->done_cnt_own);
    if (e->p_dev) hipFree(e->p_dev);
    if (e->stamps) hipFree(e->stamps);
    delete e;
    return HLX_OK;
}

int hlx_set_global_step(hlx_env* e, int64_t global_step) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_global_step: null handle");
    e->global_step = global_step;
    e->global_step_set = true;
    eval_curriculum(e);    // host only: the scalars are arguments of the next launch
    return HLX_OK;
}

int hlx_get_curriculum(hlx_env* e, double out[5]) {
    if (!e || !out) return fail(HLX_ERR_INVALID, "hlx_get_curriculum: null argument");
    memcpy(out, e->cur, sizeof e->cur);
    return HLX_OK;
}

int hlx_set_noise(hlx_env* e, const double* step_noise, const double* reset_noise) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_noise: null handle");
    e->step_noise = step_noise;
    e->reset_noise = reset_noise;
    return HLX_OK;
}

int hlx_fill_noise(hlx_env* e, double* step_noise, double* reset_noise, int32_t clock_offset, void* stream) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_fill_noise: null handle");
    HIP_TRY(hipSetDevice(e->device));
    if (e->ep_zero_pending) { int rc = pool_before_step(e, (hipStream_t)stream); if (rc) return rc; }
    hipLaunchKernelGGL(hlx_fill_noise_kernel, dim3((unsigned)((e->n + 63) / 64)), dim3(64), 0, (hipStream_t)stream,
                       step_noise, reset_noise, e->n,
                       clock_offset == 0 ? clock_arg<1>(e) : e->t + (unsigned long long)clock_offset, (uint32_t)e->seed, (uint32_t)(e->seed >> 32),
                       (long long)e->env_offset, clock_offset == 0 ? (const uint32_t*)nullptr : (const uint32_t*)e->ep_cur);
    HIP_TRY(hipGetLastError());
    return HLX_OK;
}

int hlx_reset(hlx_env* e, const uint8_t* mask, float* obs_out, void* stream) { return hlx_reset_info(e, mask, obs_out, nullptr, stream); }

int hlx_reset_info(hlx_env* e, const uint8_t* mask, float* obs_out, const hlx_info_soa* info, void* stream) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_reset: null handle");
    if (info && !info->packed) return fail(HLX_ERR_INVALID, "hlx_reset_info: reset()'s info is written in the packed form (hlx_info_soa.packed) only");
    HIP_TRY(hipSetDevice(e->device));
    KOpt want = e->p.hot.opt;
    memset(&want.info, 0, sizeof want.info);      // (a plain reset writes no info, whatever the last step wrote)
    if (info) want.info.packed = info->packed;
    want.reset_mask = mask; want.step_noise = e->step_noise; want.reset_noise = e->reset_noise;
    int rc = sync_params(e, want, (hipStream_t)stream);
    if (rc) return rc;
    KIo io{nullptr, obs_out, nullptr, nullptr, nullptr};
    if (e->t != e->epoch_t) { e->epoch_t = e->t; e->reset_epoch = 0; }     // the first reset at this clock value
    if (e->ep_zero_pending) { rc = pool_before_step(e, (hipStream_t)stream); if (rc) return rc; }
    HIP_TRY(launch<1>(e, io, (hipStream_t)stream));
    e->reset_epoch = (e->reset_epoch + 1) & 0xFFFFu;
    e->pool_dirty = true;     // (domain randomisation: the constants an episode starts from accumulate over resets)
    return HLX_OK;
}

int hlx_set_reset_epoch(hlx_env* e, uint32_t epoch) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_reset_epoch: null handle");
    if (epoch > 0xFFFFu) return fail(HLX_ERR_INVALID, "hlx_set_reset_epoch: the epoch has 16 bits (got %u)", epoch);
    e->reset_epoch = epoch; e->epoch_t = e->t;
    return HLX_OK;
}
uint32_t hlx_get_reset_epoch(const hlx_env* e) { return e ? cur_epoch(e) : 0u; }

int hlx_set_seed(hlx_env* e, uint64_t seed) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_seed: null handle");
    e->seed = seed;     // a kernel argument: in force from the next launch on; the clock keeps running
    e->p.seed_lo = (uint32_t)seed; e->p.seed_hi = (uint32_t)(seed >> 32);
    e->reset_epoch = 0; e->epoch_t = e->t;
    e->pool_dirty = true; e->ep_zero_pending = true;     // the environments' episode counters restart with the new key
    return HLX_OK;
}

int hlx_set_episode_pool(hlx_env* e, int32_t interval) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_episode_pool: null handle");
    if (interval < -1) return fail(HLX_ERR_INVALID, "hlx_set_episode_pool: interval must be -1 (default), 0 (off) or > 0");
    if (interval == 0) { e->pool_on = false; return HLX_OK; }
    if (!e->pool_on) e->pool_dirty = true;      // (entries consumed while it was off were not listed)
    e->pool_on = true;
    e->pool_interval = interval < 0 ? HLX_POOL_INTERVAL_DEFAULT : interval;
    return HLX_OK;
}
int32_t hlx_get_episode_pool(const hlx_env* e) { return e ? (e->pool_on ? e->pool_interval : 0) : -1; }
int hlx_get_episode_pool_misses(hlx_env* e, int64_t* misses) {
    if (!e || !misses) return fail(HLX_ERR_INVALID, "hlx_get_episode_pool_misses: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    int32_t v = 0;
    HIP_TRY(hipMemcpy(&v, e->rf_cnt + 2, sizeof v, hipMemcpyDeviceToHost));
    *misses = (int64_t)(uint32_t)v;
    return HLX_OK;
}

int hlx_get_episode_pool_crowded(hlx_env* e, int64_t* crowded) {
    if (!e || !crowded) return fail(HLX_ERR_INVALID, "hlx_get_episode_pool_crowded: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    int32_t v = 0;
    HIP_TRY(hipMemcpy(&v, e->rf_cnt + 3, sizeof v, hipMemcpyDeviceToHost));
    *crowded = (int64_t)(uint32_t)v;
    return HLX_OK;
}

int hlx_get_episode_pool_stats(hlx_env* e, int64_t out[4]) {
    if (!e || !out) return fail(HLX_ERR_INVALID, "hlx_get_episode_pool_stats: null argument");
    int rc = hlx_get_episode_pool_misses(e, &out[0]);
    if (rc) return rc;
    out[1] = e->pool_full_fills; out[2] = e->pool_partial_fills; out[3] = e->pool_suspended_steps;
    return HLX_OK;
}

int hlx_set_load_schedule(hlx_env* e, int32_t mode) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_load_schedule: null handle");
    if (mode < -1 || mode > 2) return fail(HLX_ERR_INVALID, "hlx_set_load_schedule: mode must be -1 (auto), 0, 1 or 2");
    if (mode < 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0) cus = 256;
        const int blocks = (e->n + 63) / 64;
        e->load_sched = blocks <= 4 * cus ? 2 : blocks <= 8 * cus ? 1 : 0;
    } else e->load_sched = mode;
    e->pool_dirty = true;     // (entries used under another schedule were not recorded)
    return HLX_OK;
}
int32_t hlx_get_load_schedule(const hlx_env* e) { return e ? e->load_sched : -1; }

static int step_impl(hlx_env* e, const float* actions, float* obs, float* reward, uint8_t* terminated,
                     uint8_t* truncated, float* terminal_obs, int32_t* done_idx, const hlx_info_soa* info,
                     hipStream_t s, bool bracket = true) {
    KOpt want;
    memset(&want, 0, sizeof want);
    want.terminal_obs = terminal_obs; want.done_idx = done_idx;
    if (info) want.info = *info;
    want.step_noise = e->step_noise; want.reset_noise = e->reset_noise;
    if (e->pipe_partial && !e->step_noise && !e->reset_noise) {
        want.pipe_partial = e->pipe_partial; want.pipe_returns = e->pipe_returns; want.pipe_gamma = e->pipe_gamma;
        want.pipe_stride = e->pipe_stride; want.pipe_col0 = e->pipe_col0;
    }
    int rc = sync_params(e, want, s);
    if (rc) return rc;
    // (hlx_kernels.hip: under the lone-wave schedule every form of the step uses pool entries)
    rc = pool_before_step(e, s, !e->step_noise && !e->reset_noise);
    if (rc) return rc;
    e->t += 1;  // this launch's clock value
    KIo io{actions, obs, reward, terminated, truncated};
    if (e->prof && bracket) { rc = prof_event(e, s); if (rc) return rc; }
    HIP_TRY(launch<0>(e, io, s));
    if (e->prof && bracket) { rc = prof_event(e, s); if (rc) return rc; e->prof_launches += 1; }
    e->pool_since += 1;
    return HLX_OK;
}

int hlx_step(hlx_env* e, const float* actions, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated,
             float* terminal_obs, int32_t* done_idx, int32_t* n_done, const hlx_info_soa* info, void* stream) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_step: null handle");
    if (!actions || !reward || !terminated || !truncated)
        return fail(HLX_ERR_INVALID, "hlx_step: actions, reward, terminated and truncated are required");
    if ((done_idx == nullptr) != (n_done == nullptr))
        return fail(HLX_ERR_INVALID, "hlx_step: done_idx and n_done must be given together");
    if (const char* why = info_invalid(e, info)) return fail(HLX_ERR_INVALID, "hlx_step: %s", why);
    HIP_TRY(hipSetDevice(e->device));
    int rc = step_impl(e, actions, obs, reward, terminated, truncated, terminal_obs, done_idx, info, (hipStream_t)stream);
    if (rc) return rc;
    if (n_done && n_done != e->done_cnt + (e->t & 1ull))    // (a caller that owns the counter reads it in place: hlx_set_done_counter)
        HIP_TRY(hipMemcpyAsync(n_done, e->done_cnt + (e->t & 1ull), sizeof(int32_t), hipMemcpyDeviceToDevice,
                               (hipStream_t)stream));
    return HLX_OK;
}

int hlx_rollout(hlx_env* e, const float* actions, int32_t T, int32_t out_slots, float* obs, float* reward,
                uint8_t* terminated, uint8_t* truncated, void* stream) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_rollout: null handle");
    if (!actions || !reward || !terminated || !truncated || T < 0 || out_slots < 1)
        return fail(HLX_ERR_INVALID, "hlx_rollout: bad argument");
    HIP_TRY(hipSetDevice(e->device));
    const size_t N = (size_t)e->n;
    // profiling: ONE event pair around the back-to-back launch train (an event between every two launches would itself
    // open a gap).  In the one-launch-per-step form the first event is recorded BEHIND the first launch and the pair
    // covers the T - 1 launches that follow it: an event recorded ahead of the train completes the moment it reaches an idle
    // GPU, a launch latency before the first kernel starts, and a short train (T = 20) would be charged that gap as
    // kernel time (measured: 10.8 us against 9.7 us per launch).
    const bool fused_form = e->rollout_chunk > 1 && !e->step_noise && !e->reset_noise;
    if (e->prof && T > 0 && (fused_form || T == 1)) { int rc = prof_event(e, (hipStream_t)stream); if (rc) return rc; }
    if (e->rollout_chunk > 1 && !e->step_noise && !e->reset_noise) {
        // fused rollout: up to `rollout_chunk` steps per launch, the environments' state stays in registers in between
        KOpt want;
        memset(&want, 0, sizeof want);
        int rc = sync_params(e, want, (hipStream_t)stream);
        if (rc) return rc;
        rc = pool_before_step(e, (hipStream_t)stream);
        if (rc) return rc;
        for (int32_t k = 0; k < T; k += e->rollout_chunk) {
            const int32_t steps = std::min<int32_t>(e->rollout_chunk, T - k);
            e->t += 1;   // clock of the first step of this launch
            KIo io{actions + (size_t)k * N * HLX_ACT_DIM, obs, reward, terminated, truncated};
            HIP_TRY(launch_fused(e, io, steps, (int)(k % out_slots), out_slots, (hipStream_t)stream));
            e->t += (unsigned long long)(steps - 1);
        }
        if (T > 0) e->pool_dirty = true;     // the fused kernel consumes episodes without listing them: every entry is renewed before the next step launch
        if (e->prof && T > 0) { rc = prof_event(e, (hipStream_t)stream); if (rc) return rc; e->prof_launches += T; }
        return HLX_OK;
    }
    for (int32_t k = 0; k < T; ++k) {
        const size_t slot = (size_t)(k % out_slots);
        int rc = step_impl(e, actions + (size_t)k * N * HLX_ACT_DIM, obs ? obs + slot * N * HLX_OBS_DIM : nullptr,
                           reward + slot * N, terminated + slot * N, truncated + slot * N, e->rollout_terminal, e->rollout_done_idx,
                           e->rollout_has_info ? &e->rollout_info : nullptr, (hipStream_t)stream, false);
        if (rc) return rc;
        if (e->prof && k == 0 && T > 1) { rc = prof_event(e, (hipStream_t)stream); if (rc) return rc; }
    }
    if (e->prof && T > 0) { int rc = prof_event(e, (hipStream_t)stream); if (rc) return rc; e->prof_launches += (T > 1 ? T - 1 : T); }
    return HLX_OK;
}

int hlx_set_rollout_terminal_obs(hlx_env* e, float* terminal_obs) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_rollout_terminal_obs: null handle");
    e->rollout_terminal = terminal_obs;
    return HLX_OK;
}

int hlx_set_rollout_outputs(hlx_env* e, float* terminal_obs, int32_t* done_idx, const hlx_info_soa* info) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_rollout_outputs: null handle");
    if (const char* why = info_invalid(e, info)) return fail(HLX_ERR_INVALID, "hlx_set_rollout_outputs: %s", why);
    e->rollout_terminal = terminal_obs;
    e->rollout_done_idx = done_idx;
    e->rollout_has_info = info != nullptr;
    if (info) e->rollout_info = *info; else memset(&e->rollout_info, 0, sizeof e->rollout_info);
    return HLX_OK;
}

int hlx_set_done_counter(hlx_env* e, int32_t* counter2) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_done_counter: null handle");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());      // a configuration call: no launch of this handle may still be counting
    int32_t* want = counter2 ? counter2 : e->done_cnt_own;
    HIP_TRY(hipMemset(want, 0, 2 * sizeof(int32_t)));
    e->done_cnt = want;
    e->p.done_cnt = want;
    HIP_TRY(hipMemcpy(reinterpret_cast<char*>(e->p_dev) + offsetof(KParams, done_cnt), &e->p.done_cnt, sizeof(int32_t*), hipMemcpyHostToDevice));
    return HLX_OK;
}

int hlx_set_rollout_fused(hlx_env* e, int32_t steps_per_launch) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_set_rollout_fused: null handle");
    if (steps_per_launch < 1) return fail(HLX_ERR_INVALID, "hlx_set_rollout_fused: steps_per_launch must be >= 1");
    e->rollout_chunk = steps_per_launch;
    return HLX_OK;
}

int hlx_profile(hlx_env* e, int32_t enable) {
    if (!e) return fail(HLX_ERR_INVALID, "hlx_profile: null handle");
    e->prof = enable != 0;
    e->ev_used = 0;
    e->prof_launches = 0;
    return HLX_OK;
}

int hlx_profile_read(hlx_env* e, double* total_ms, int64_t* launches) {
    if (!e || !total_ms || !launches) return fail(HLX_ERR_INVALID, "hlx_profile_read: null argument");
    HIP_TRY(hipSetDevice(e->device));
    double sum = 0.0;
    const size_t pairs = e->ev_used / 2;
    if (pairs) HIP_TRY(hipEventSynchronize(e->ev_pool[e->ev_used - 1]));
    for (size_t p = 0; p < pairs; ++p) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev_pool[2 * p], e->ev_pool[2 * p + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *launches = e->prof_launches;
    e->ev_used = 0;
    e->prof_launches = 0;
    return HLX_OK;
}

// ---- logical state export / injection -------------------------------------------------------------
namespace {
struct Planes {
    size_t N, NB, g_planes, o_planes;
    int g_cap, o_cap;
    std::vector<float4> h;
    float4* G;
    float4* O;
};
void planes_init(const hlx_env* e, Planes& p) {
    p.N = (size_t)e->n;
    p.g_cap = e->k.g_delay + 1; p.o_cap = e->k.o_cap;
    p.g_planes = (size_t)((e->cfg.flags & HLX_F_GROUND) ? p.g_cap * GROUND_RING_WORDS16 : 0);
    p.o_planes = (size_t)(e->k.o_delay > 0 ? p.o_cap : 0);
    p.NB = ((p.N + 63) / 64) * 64;
    p.h.resize(p.NB * N_GROUPS + p.N * (p.g_planes + p.o_planes));
    p.G = p.h.data() + p.NB * N_GROUPS;
    p.O = p.G + p.N * p.g_planes;
}
}  // namespace

int hlx_get_state(hlx_env* e, hlx_env_state* out) {
    if (!e || !out) return fail(HLX_ERR_INVALID, "hlx_get_state: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    Planes p;
    planes_init(e, p);
    const size_t N = p.N;
    HIP_TRY(hipMemcpy(p.h.data(), e->arena, sizeof(float4) * p.h.size(), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ep(N);
    if (e->ep_zero_pending) std::fill(ep.begin(), ep.end(), 0u);
    else HIP_TRY(hipMemcpy(ep.data(), e->ep_cur, sizeof(uint32_t) * N, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) {
        hlx_env_state& s = out[i];
        memset(&s, 0, sizeof s);
        auto g = [&](int grp) { return p.h[((i / 64) * N_GROUPS + (size_t)grp) * 64 + (i % 64)]; };
        float4 v = g(G_IPOS); s.int_pos[0] = v.x; s.int_pos[1] = v.y; s.int_pos[2] = v.z; s.fuel = v.w;
        v = g(G_IVEL); s.int_vel[0] = v.x; s.int_vel[1] = v.y; s.int_vel[2] = v.z; s.prev_distance = v.w;
        v = g(G_QUAT); s.int_quat[0] = v.x; s.int_quat[1] = v.y; s.int_quat[2] = v.z; s.int_quat[3] = v.w;
        v = g(G_MPOS); s.mis_pos[0] = v.x; s.mis_pos[1] = v.y; s.mis_pos[2] = v.z; s.min_distance = v.w;
        v = g(G_MVEL); s.mis_vel[0] = v.x; s.mis_vel[1] = v.y; s.mis_vel[2] = v.z; s.last_distance = v.w;
        v = g(G_W0); s.wind[0] = f4_as_d(v.x, v.y); s.wind[1] = f4_as_d(v.z, v.w);
        v = g(G_W1); s.wind[2] = f4_as_d(v.x, v.y); s.ep_return = v.w;
        uint32_t packed; memcpy(&packed, &v.z, 4);
        s.steps = (int32_t)(packed & 0x1FFFu); s.worsening = (int32_t)((packed >> 13) & 0xFFFu);
        s.crossed = (packed >> 25) & 1u; s.kf_init = (packed >> 26) & 1u; s.kf_x_is64 = (packed >> 27) & 1u;
        s.on_delay = (int32_t)(packed >> 28);
        s.episode = (int32_t)ep[i];
        v = g(G_KF0); s.kf_x[0] = f4_as_d(v.x, v.y); s.kf_x[1] = f4_as_d(v.z, v.w);
        v = g(G_KF1); s.kf_x[2] = f4_as_d(v.x, v.y); s.kf_x[3] = f4_as_d(v.z, v.w);
        v = g(G_KF2); s.kf_x[4] = f4_as_d(v.x, v.y); s.kf_x[5] = f4_as_d(v.z, v.w);
        v = g(G_KFP); s.kf_P[0] = v.x; s.kf_P[1] = v.y; s.kf_P[2] = v.z; s.kf_P[3] = v.w;
        v = g(G_THRUST); s.thrust_actual[0] = v.x; s.thrust_actual[1] = v.y; s.thrust_actual[2] = v.z; s.cd_super = v.w;
        v = g(G_MISC); s.T0 = f4_as_d(v.x, v.y); s.base_cd = v.z; s.transonic_peak_m1 = v.w;
        s.fuel_used = reinterpret_cast<const float*>(&p.h[((i / 64) * N_GROUPS + (size_t)G_AUX) * 64])[i % 64];     // a plane of dwords
        for (int k = 0; k < e->k.volley_k; ++k) {
            v = g(G_VPOS + k); s.v_pos[k][0] = v.x; s.v_pos[k][1] = v.y; s.v_pos[k][2] = v.z; s.v_min[k] = v.w;
            v = g(G_VVEL + k); s.v_vel[k][0] = v.x; s.v_vel[k][1] = v.y; s.v_vel[k][2] = v.z;
            uint32_t w; memcpy(&w, &v.w, 4);
            s.v_active[k] = (int32_t)(w & 1u);
            if (k == 0) { s.prio = (int32_t)((w >> 8) & 3u); s.n_intercepted = (int32_t)((w >> 12) & 7u); }
        }
        if (e->k.o_delay > 0) {
            int len = s.steps + 1 < s.on_delay + 1 ? s.steps + 1 : s.on_delay + 1;
            s.on_len = len;
            for (int k = 0; k < len; ++k) {
                unsigned long long tau = e->t - (unsigned long long)(len - 1 - k);
                float4 r = p.O[(size_t)(tau % (unsigned long long)p.o_cap) * N + i];
                s.on_ring[k][0] = r.x; s.on_ring[k][1] = r.y; s.on_ring[k][2] = r.z; s.on_ring[k][3] = r.w;
            }
        }
        if (e->k.g_delay > 0) {
            int len = s.steps + 1 < p.g_cap ? s.steps + 1 : p.g_cap;
            s.g_len = len;
            for (int k = 0; k < len; ++k) {
                unsigned long long tau = e->t - (unsigned long long)(len - 1 - k);
                size_t slot = (size_t)(tau % (unsigned long long)p.g_cap);
                float4 r0 = p.G[(slot * 3) * N + i], r1 = p.G[(slot * 3 + 1) * N + i], r2 = p.G[(slot * 3 + 2) * N + i];
                double* d = s.g_ring[k];
                d[0] = f4_as_d(r0.x, r0.y); d[1] = f4_as_d(r0.z, r0.w); d[2] = f4_as_d(r1.x, r1.y);
                d[3] = r1.z; d[4] = r2.x; d[5] = r2.y; d[6] = r2.z; d[7] = r1.w;
            }
        }
    }
    return HLX_OK;
}

int hlx_set_state(hlx_env* e, const hlx_env_state* in) {
    if (!e || !in) return fail(HLX_ERR_INVALID, "hlx_set_state: null argument");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    Planes p;
    planes_init(e, p);
    const size_t N = p.N;
    HIP_TRY(hipMemcpy(p.h.data(), e->arena, sizeof(float4) * p.h.size(), hipMemcpyDeviceToHost));
    std::vector<uint32_t> ep(N);
    for (size_t i = 0; i < N; ++i) ep[i] = (uint32_t)in[i].episode;
    for (size_t i = 0; i < N; ++i) {
        const hlx_env_state& s = in[i];
        if (s.steps < 0 || s.steps > HLX_MAX_STEPS || s.on_delay < 0 || s.on_delay > HLX_MAX_DELAY)
            return fail(HLX_ERR_INVALID, "hlx_set_state: env %zu has steps/on_delay out of range", i);
        auto put = [&](int grp, float4 v) { p.h[((i / 64) * N_GROUPS + (size_t)grp) * 64 + (i % 64)] = v; };
        uint32_t packed = (uint32_t)s.steps | ((uint32_t)(s.worsening > 0xFFF ? 0xFFF : (s.worsening < 0 ? 0 : s.worsening)) << 13) |
                          ((uint32_t)(s.crossed != 0) << 25) | ((uint32_t)(s.kf_init != 0) << 26) |
                          ((uint32_t)(s.kf_x_is64 != 0) << 27) | ((uint32_t)s.on_delay << 28);
        float pw; memcpy(&pw, &packed, 4);
        float4 v;
        put(G_IPOS, make_float4(s.int_pos[0], s.int_pos[1], s.int_pos[2], s.fuel));
        put(G_IVEL, make_float4(s.int_vel[0], s.int_vel[1], s.int_vel[2], s.prev_distance));
        put(G_QUAT, make_float4(s.int_quat[0], s.int_quat[1], s.int_quat[2], s.int_quat[3]));
        put(G_MPOS, make_float4(s.mis_pos[0], s.mis_pos[1], s.mis_pos[2], s.min_distance));
        put(G_MVEL, make_float4(s.mis_vel[0], s.mis_vel[1], s.mis_vel[2], s.last_distance));
        d_as_f2(s.wind[0], v.x, v.y); d_as_f2(s.wind[1], v.z, v.w); put(G_W0, v);
        d_as_f2(s.wind[2], v.x, v.y); v.z = pw; v.w = s.ep_return; put(G_W1, v);
        d_as_f2(s.kf_x[0], v.x, v.y); d_as_f2(s.kf_x[1], v.z, v.w); put(G_KF0, v);
        d_as_f2(s.kf_x[2], v.x, v.y); d_as_f2(s.kf_x[3], v.z, v.w); put(G_KF1, v);
        d_as_f2(s.kf_x[4], v.x, v.y); d_as_f2(s.kf_x[5], v.z, v.w); put(G_KF2, v);
        put(G_KFP, make_float4(s.kf_P[0], s.kf_P[1], s.kf_P[2], s.kf_P[3]));
        put(G_THRUST, make_float4(s.thrust_actual[0], s.thrust_actual[1], s.thrust_actual[2], s.cd_super));
        d_as_f2(s.T0, v.x, v.y); v.z = s.base_cd; v.w = s.transonic_peak_m1; put(G_MISC, v);
        reinterpret_cast<float*>(&p.h[((i / 64) * N_GROUPS + (size_t)G_AUX) * 64])[i % 64] = s.fuel_used;
        for (int k = 0; k < e->k.volley_k; ++k) {
            if (k == 0 && (s.prio < 0 || s.prio >= e->k.volley_k || s.n_intercepted < 0 || s.n_intercepted > HLX_MAX_VOLLEY))
                return fail(HLX_ERR_INVALID, "hlx_set_state: env %zu has prio/n_intercepted out of range", i);
            const uint32_t w = (uint32_t)(s.v_active[k] != 0) | (k == 0 ? ((uint32_t)s.prio << 8) | ((uint32_t)s.n_intercepted << 12) : 0u);
            float fw; memcpy(&fw, &w, 4);
            put(G_VPOS + k, make_float4(s.v_pos[k][0], s.v_pos[k][1], s.v_pos[k][2], s.v_min[k]));
            put(G_VVEL + k, make_float4(s.v_vel[k][0], s.v_vel[k][1], s.v_vel[k][2], fw));
        }
        if (e->k.o_delay > 0) {
            int len = s.on_len;
            for (int k = 0; k < len && k < HLX_RING_CAP; ++k) {
                unsigned long long tau = e->t - (unsigned long long)(len - 1 - k);
                p.O[(size_t)(tau % (unsigned long long)p.o_cap) * N + i] =
                    make_float4(s.on_ring[k][0], s.on_ring[k][1], s.on_ring[k][2], s.on_ring[k][3]);
            }
        }
        if (e->k.g_delay > 0) {
            int len = s.g_len;
            for (int k = 0; k < len && k < HLX_RING_CAP; ++k) {
                unsigned long long tau = e->t - (unsigned long long)(len - 1 - k);
                size_t slot = (size_t)(tau % (unsigned long long)p.g_cap);
                const double* d = s.g_ring[k];
                float4 r0, r1;
                d_as_f2(d[0], r0.x, r0.y); d_as_f2(d[1], r0.z, r0.w); d_as_f2(d[2], r1.x, r1.y);
                r1.z = (float)d[3]; r1.w = (float)d[7];
                p.G[(slot * 3) * N + i] = r0;
                p.G[(slot * 3 + 1) * N + i] = r1;
                p.G[(slot * 3 + 2) * N + i] = make_float4((float)d[4], (float)d[5], (float)d[6], 0.f);
            }
        }
    }
    HIP_TRY(hipMemcpy(e->arena, p.h.data(), sizeof(float4) * p.h.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->ep_cur, ep.data(), sizeof(uint32_t) * N, hipMemcpyHostToDevice));
    e->ep_zero_pending = false;
    e->pool_dirty = true;     // prepared episodes were computed from the state that has just been replaced
    return HLX_OK;
}

#ifdef HLX_STAMPS
// diagnostic build only: s_memtime samples of the last launch, [blocks][16]
int hlx_debug_read_stamps(hlx_env* e, unsigned long long* host_out) {
    if (!e || !host_out || !e->stamps) return fail(HLX_ERR_INVALID, "hlx_debug_read_stamps: no stamp buffer");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, e->stamps, sizeof(unsigned long long) * 16 * ((size_t)(e->n + 63) / 64), hipMemcpyDeviceToHost));
    return HLX_OK;
}
#endif

}  // extern "C"
