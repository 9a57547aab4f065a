// hlx_eval.inc -- closed-loop evaluation of the classical guidance laws (C ABI: include/hlx_eval.h; included by hlx_kernels.hip).
//
// One lane per environment, 256-thread blocks, one small launch behind every step launch.  Per environment-step it reads
// the step's outputs it needs (reward, the two done bytes, two float2 of the observation row -- four where a law runs --,
// two of the terminal row where the environment finished, and the positions / intercepted bit of the info words), reads
// and writes 40 bytes of accumulators, and stores the next action with three float2 stores.  Arithmetic follows the
// reference's numpy 2 dtypes (tests/guidance_ref.py restates it; tests/golden/guidance/ pins it bit for bit).
#include "../../include/hlx_eval.h"

namespace {

struct EvalK {
    int n, E, use_true;
    float N, K, kill;            // float32 forms: a Python float next to a float32 value rounds to float32 (NEP 50)
    double Kd;                   // APN's first lock call: the previous rate is still float64 zeros, the gain term float64
    float4* accf;                // fuel at reset, min distance, final distance, total reward
    int4* acci;                  // steps, lock losses, lock recoveries, (episode index << 2) | APN rate is float32 << 1 | was_locked
    float2* prev;                // APN previous line-of-sight rates
    float *r_mind, *r_final, *r_ret, *r_fuel;      // records [E][n]
    int32_t *r_steps, *r_loss, *r_rec;
    uint8_t* r_success;
    int32_t* count;              // environments that have written their E-th record
};

struct EvalIo {
    const float* obs;
    const float* reward;
    const uint8_t *term, *trunc;
    const float* terminal_obs;
    const float *ip, *mp;        // [3][n] planes (PACKED == false)
    const uint8_t* flags;
    const float4* packed;        // hlx_info_soa.packed [3][n] words (PACKED == true)
    float* actions;
};

// observation rows are 104 B: a row starts 8-byte aligned, so even-indexed pairs load as float2
DEV float2 ld2(const float* row, int j) { return *reinterpret_cast<const float2*>(row + j); }
DEV float clip1(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }     // np.clip: NaN stays NaN

// get_action of the three laws (paper_benchmark_suite.py:92-195) on o[0:4] and o[14]; pv / fl: the APN state
template <int LAW>
DEV void eval_action(const EvalK& k, float2 o01, float2 o23, float o14, float2& pv, int& fl, float* __restrict__ out) {
    float a0 = 1.0f, a1 = 0.0f, a2 = 0.0f;
    if (o14 < 0.3f) {                                                        // coast (:114, :145, :177)
        a0 = 0.3f;
    } else if (LAW == HLX_LAW_PURSUIT) {                                     // :180-195
        const float nrm = snorm3(v3(o01.x, o01.y, o23.x));
        if (!(nrm < 1e-6f)) { a1 = o01.y / nrm; a2 = o23.x / nrm; }          // IEEE float32 division; not clipped
    } else {
        float az = o23.x, el = o23.y;
        if (!(LAW == HLX_LAW_PN && k.use_true)) { az = az * 0.5f; el = el * 0.5f; }
        if (LAW == HLX_LAW_PN) {                                             // :119-132
            a1 = k.N * az;
            a2 = k.N * el;
        } else if (fl & 2) {                                                 // :148-166, float32 previous rate
            a1 = k.N * az + k.K * (az - pv.x);
            a2 = k.N * el + k.K * (el - pv.y);
        } else {                                                             // first lock call: float64 zeros as previous rate
            a1 = (float)((double)(k.N * az) + k.Kd * ((double)az - 0.0));
            a2 = (float)((double)(k.N * el) + k.Kd * ((double)el - 0.0));
        }
        if (LAW == HLX_LAW_APN) { pv = make_float2(az, el); fl |= 2; }
        a1 = clip1(a1);
        a2 = clip1(a2);
    }
    float2* o = reinterpret_cast<float2*>(out);
    o[0] = make_float2(a0, a1);
    o[1] = make_float2(a2, 0.0f);
    o[2] = make_float2(0.0f, 0.0f);
}

template <int LAW>
__global__ __launch_bounds__(256) void hlx_eval_begin_kernel(EvalK k, const float* __restrict__ obs, float* __restrict__ actions) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k.n) return;
    const float* row = obs + (size_t)i * HLX_OBS_DIM;
    const float2 o12 = ld2(row, 12), o14 = ld2(row, 14);
    int fl = o14.x > 0.5f ? 1 : 0;                                           // initial_fuel / was_locked (:250-251)
    k.accf[i] = make_float4(o12.x, __builtin_inff(), 0.0f, 0.0f);
    float2 pv = make_float2(0.0f, 0.0f);
    if (LAW != HLX_LAW_NONE) eval_action<LAW>(k, ld2(row, 0), ld2(row, 2), o14.x, pv, fl, actions + (size_t)i * HLX_ACT_DIM);
    k.acci[i] = make_int4(0, 0, 0, fl);
    if (LAW == HLX_LAW_APN) k.prev[i] = pv;
}

template <int LAW, bool PACKED>
__global__ __launch_bounds__(256) void hlx_eval_observe_kernel(EvalK k, EvalIo io) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = k.n;
    if (i >= n) return;
    float4 af = k.accf[i];
    int4 ai = k.acci[i];
    const bool done = ((unsigned)io.term[i] | (unsigned)io.trunc[i]) != 0u;
    V3 ip, mp;
    bool hit;
    if (PACKED) {
        const float4 w1 = io.packed[n + i], w2 = io.packed[2 * n + i];
        ip = v3(w1.x, w1.y, w1.z);
        mp = v3(w2.x, w2.y, w2.z);
        hit = (__float_as_uint(w2.w) & 1u) != 0u;
    } else {
        ip = v3(io.ip[i], io.ip[n + i], io.ip[2 * n + i]);
        mp = v3(io.mp[i], io.mp[n + i], io.mp[2 * n + i]);
        hit = (io.flags[i] & 1u) != 0u;
    }
    // every load a lane needs is issued up front; only a finished lane's terminal row waits for the done bytes
    const float* cur = io.obs + (size_t)i * HLX_OBS_DIM;
    const float2 c12 = ld2(cur, 12), c14 = ld2(cur, 14);
    float2 o01 = make_float2(0.0f, 0.0f), o23 = o01, pv = o01;
    if (LAW != HLX_LAW_NONE) { o01 = ld2(cur, 0); o23 = ld2(cur, 2); }
    if (LAW == HLX_LAW_APN) pv = k.prev[i];
    // per step (:262-281): steps, reward sum, min / final distance, lock transitions.  The reference's sum starts as the Python
    // float 0.0 and becomes np.float32 with the first reward (np.float32); a Python-float terminal bonus joins it rounded to
    // float32 (NEP 50).  So it is a float32 sum in step order, which is what this is.
    const float d = snorm3(ip - mp);
    ai.x += 1;
    af.w = af.w + io.reward[i];
    af.y = d < af.y ? d : af.y;                                              // Python min(m, d)
    af.z = d;
    float2 l12 = c12, l14 = c14;
    if (done) {
        const float* last = io.terminal_obs + (size_t)i * HLX_OBS_DIM;
        l12 = ld2(last, 12);
        l14 = ld2(last, 14);
    }
    const bool locked = l14.x > 0.5f, was = (ai.w & 1) != 0;
    if (was && !locked) ai.y += 1;
    else if (!was && locked) ai.z += 1;
    ai.w = (ai.w & ~1) | (locked ? 1 : 0);
    if (done) {
        const int e = ai.w >> 2;
        if (e < k.E) {                                                       // :283-290
            const size_t s = (size_t)e * n + i;
            k.r_mind[s] = af.y;
            k.r_final[s] = af.z;
            k.r_steps[s] = ai.x;
            k.r_ret[s] = af.w;
            k.r_fuel[s] = af.x - l12.x;
            k.r_loss[s] = ai.y;
            k.r_rec[s] = ai.z;
            k.r_success[s] = (uint8_t)((hit || af.y < k.kill) ? 1 : 0);
            if (e + 1 == k.E) atomicAdd(k.count, 1);
        }
        // the auto-reset observation starts the next episode
        af = make_float4(c12.x, __builtin_inff(), 0.0f, 0.0f);
        ai = make_int4(0, 0, 0, ((e + 1) << 2) | (ai.w & 2) | (c14.x > 0.5f ? 1 : 0));
    }
    if (LAW != HLX_LAW_NONE) {
        int fl = ai.w;
        eval_action<LAW>(k, o01, o23, c14.x, pv, fl, io.actions + (size_t)i * HLX_ACT_DIM);
        ai.w = fl;
        if (LAW == HLX_LAW_APN) k.prev[i] = pv;
    }
    k.accf[i] = af;
    k.acci[i] = ai;
}

}  // namespace

struct hlx_eval {
    hlx_eval_config c;
    EvalK k;
    void* mem;                   // one allocation: accumulators, records, counter, the run buffers
    float *obs, *reward, *terminal_obs, *actions;
    uint8_t *term, *trunc;
    float4* packed;
    int32_t* count_host;         // pinned
};

namespace {

template <int LAW>
hipError_t eval_begin_as(const hlx_eval* ev, const float* obs, float* actions, hipStream_t s) {
    hipLaunchKernelGGL((hlx_eval_begin_kernel<LAW>), dim3((ev->k.n + 255) / 256), dim3(256), 0, s, ev->k, obs, actions);
    return hipGetLastError();
}

template <int LAW>
hipError_t eval_observe_as(const hlx_eval* ev, const EvalIo& io, hipStream_t s) {
    const dim3 grid((ev->k.n + 255) / 256);
    if (io.packed) hipLaunchKernelGGL((hlx_eval_observe_kernel<LAW, true>), grid, dim3(256), 0, s, ev->k, io);
    else hipLaunchKernelGGL((hlx_eval_observe_kernel<LAW, false>), grid, dim3(256), 0, s, ev->k, io);
    return hipGetLastError();
}

int eval_begin(hlx_eval* ev, const float* obs, float* actions, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(ev->k.count, 0, sizeof(int32_t), s));
    switch (ev->c.law) {
        case HLX_LAW_PURSUIT: HIP_TRY(eval_begin_as<HLX_LAW_PURSUIT>(ev, obs, actions, s)); break;
        case HLX_LAW_PN: HIP_TRY(eval_begin_as<HLX_LAW_PN>(ev, obs, actions, s)); break;
        case HLX_LAW_APN: HIP_TRY(eval_begin_as<HLX_LAW_APN>(ev, obs, actions, s)); break;
        default: HIP_TRY(eval_begin_as<HLX_LAW_NONE>(ev, obs, actions, s)); break;
    }
    return HLX_OK;
}

int eval_observe(hlx_eval* ev, const EvalIo& io, hipStream_t s) {
    switch (ev->c.law) {
        case HLX_LAW_PURSUIT: HIP_TRY(eval_observe_as<HLX_LAW_PURSUIT>(ev, io, s)); break;
        case HLX_LAW_PN: HIP_TRY(eval_observe_as<HLX_LAW_PN>(ev, io, s)); break;
        case HLX_LAW_APN: HIP_TRY(eval_observe_as<HLX_LAW_APN>(ev, io, s)); break;
        default: HIP_TRY(eval_observe_as<HLX_LAW_NONE>(ev, io, s)); break;
    }
    return HLX_OK;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the kernels read observation rows and write action rows as float2, the packed info words as float4
bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" {

int hlx_eval_destroy(hlx_eval* ev) {
    if (!ev) return HLX_OK;
    (void)hipSetDevice(ev->c.device);
    (void)hipDeviceSynchronize();
    if (ev->mem) (void)hipFree(ev->mem);
    if (ev->count_host) (void)hipHostFree(ev->count_host);
    delete ev;
    return HLX_OK;
}

int hlx_eval_create(const hlx_eval_config* cfg, hlx_eval** out) {
    if (!cfg || !out) return fail(HLX_ERR_INVALID, "hlx_eval_create: null argument");
    if (cfg->n_envs < 1) return fail(HLX_ERR_INVALID, "hlx_eval_create: n_envs must be >= 1 (got %d)", cfg->n_envs);
    if (cfg->law < HLX_LAW_NONE || cfg->law > HLX_LAW_APN) return fail(HLX_ERR_INVALID, "hlx_eval_create: law %d is not an HLX_LAW_*", cfg->law);
    if (cfg->episodes_per_env < 1) return fail(HLX_ERR_INVALID, "hlx_eval_create: episodes_per_env must be >= 1 (got %d)", cfg->episodes_per_env);
    if ((int64_t)cfg->episodes_per_env * cfg->n_envs > ((int64_t)1 << 31))
        return fail(HLX_ERR_INVALID, "hlx_eval_create: episodes_per_env x n_envs exceeds 2^31 records");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(HLX_ERR_INVALID, "hlx_eval_create: device %d not in [0, %d)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    hlx_eval* ev = new (std::nothrow) hlx_eval();
    if (!ev) return fail(HLX_ERR_NOMEM, "hlx_eval_create: out of host memory");
    ev->c = *cfg;
    const size_t N = (size_t)cfg->n_envs, R = (size_t)cfg->episodes_per_env * N;
    // layout: accf | acci | prev | 7 x 4-byte record planes | success | count | obs | terminal_obs | reward | term | trunc | packed | actions
    size_t off[16], o = 0;
    const size_t sizes[16] = {16 * N, 16 * N, 8 * N, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R, 4 * R, R, 4,
                              4 * HLX_OBS_DIM * N, 4 * HLX_OBS_DIM * N, 4 * N, 2 * align256(N) + 48 * N + 24 * N};
    for (int j = 0; j < 16; ++j) { off[j] = o; o += align256(sizes[j]); }
    hipError_t err = hipMalloc(&ev->mem, o);
    if (err == hipSuccess) err = hipMemset(ev->mem, 0, o);
    if (err == hipSuccess) err = hipHostMalloc((void**)&ev->count_host, sizeof(int32_t), hipHostMallocDefault);
    if (err != hipSuccess) {
        int rc = fail(err == hipErrorOutOfMemory ? HLX_ERR_NOMEM : HLX_ERR_HIP, "hlx_eval_create: %s", hipGetErrorString(err));
        hlx_eval_destroy(ev);
        return rc;
    }
    char* b = (char*)ev->mem;
    EvalK& k = ev->k;
    k.n = cfg->n_envs; k.E = cfg->episodes_per_env; k.use_true = cfg->use_true_state != 0;
    k.N = (float)cfg->N; k.K = (float)cfg->K_acc; k.kill = (float)cfg->kill_radius; k.Kd = cfg->K_acc;
    k.accf = (float4*)(b + off[0]); k.acci = (int4*)(b + off[1]); k.prev = (float2*)(b + off[2]);
    k.r_mind = (float*)(b + off[3]); k.r_final = (float*)(b + off[4]); k.r_ret = (float*)(b + off[5]); k.r_fuel = (float*)(b + off[6]);
    k.r_steps = (int32_t*)(b + off[7]); k.r_loss = (int32_t*)(b + off[8]); k.r_rec = (int32_t*)(b + off[9]);
    k.r_success = (uint8_t*)(b + off[10]); k.count = (int32_t*)(b + off[11]);
    ev->obs = (float*)(b + off[12]); ev->terminal_obs = (float*)(b + off[13]); ev->reward = (float*)(b + off[14]);
    char* tail = b + off[15];
    ev->term = (uint8_t*)tail; ev->trunc = (uint8_t*)(tail + align256(N));
    ev->packed = (float4*)(tail + 2 * align256(N));
    ev->actions = (float*)(tail + 2 * align256(N) + 48 * N);
    *out = ev;
    return HLX_OK;
}

int hlx_eval_begin(hlx_eval* ev, const float* obs, float* actions_out, void* stream) {
    if (!ev || !obs) return fail(HLX_ERR_INVALID, "hlx_eval_begin: null argument");
    if (misaligned(obs, 8) || misaligned(actions_out, 8)) return fail(HLX_ERR_INVALID, "hlx_eval_begin: obs and actions_out must be 8-byte aligned");
    if (ev->c.law != HLX_LAW_NONE && !actions_out) return fail(HLX_ERR_INVALID, "hlx_eval_begin: this law writes actions: actions_out is required");
    HIP_TRY(hipSetDevice(ev->c.device));
    return eval_begin(ev, obs, actions_out, (hipStream_t)stream);
}

int hlx_eval_observe(hlx_eval* ev, const float* obs, const float* reward, const uint8_t* terminated, const uint8_t* truncated,
                     const float* terminal_obs, const hlx_info_soa* info, float* actions_out, void* stream) {
    if (!ev || !obs || !reward || !terminated || !truncated || !terminal_obs || !info)
        return fail(HLX_ERR_INVALID, "hlx_eval_observe: obs, reward, terminated, truncated, terminal_obs and info are required");
    if (!info->packed && (!info->interceptor_pos || !info->missile_pos || !info->flags))
        return fail(HLX_ERR_INVALID, "hlx_eval_observe: info needs `packed`, or interceptor_pos, missile_pos and flags");
    if (ev->c.law != HLX_LAW_NONE && !actions_out) return fail(HLX_ERR_INVALID, "hlx_eval_observe: this law writes actions: actions_out is required");
    if (misaligned(obs, 8) || misaligned(terminal_obs, 8) || misaligned(actions_out, 8) || misaligned(info->packed, 16))
        return fail(HLX_ERR_INVALID, "hlx_eval_observe: obs, terminal_obs and actions_out must be 8-byte aligned, info->packed 16-byte aligned");
    HIP_TRY(hipSetDevice(ev->c.device));
    EvalIo io{obs, reward, terminated, truncated, terminal_obs, info->interceptor_pos, info->missile_pos, info->flags,
              (const float4*)info->packed, actions_out};
    return eval_observe(ev, io, (hipStream_t)stream);
}

int hlx_eval_run(hlx_eval* ev, hlx_env* env, int32_t max_steps, int32_t check_every, float* action_tape, int64_t* steps_run, void* stream) {
    if (steps_run) *steps_run = 0;
    if (!ev || !env) return fail(HLX_ERR_INVALID, "hlx_eval_run: null handle");
    if (ev->c.law == HLX_LAW_NONE) return fail(HLX_ERR_INVALID, "hlx_eval_run: needs a law (HLX_LAW_NONE is driven with hlx_eval_observe)");
    if (env->n != ev->c.n_envs || env->device != ev->c.device)
        return fail(HLX_ERR_INVALID, "hlx_eval_run: the environment handle has %d environments on device %d, the evaluator %d on %d",
                    env->n, env->device, ev->c.n_envs, ev->c.device);
    if (max_steps < 0 || check_every < 1) return fail(HLX_ERR_INVALID, "hlx_eval_run: need max_steps >= 0 and check_every >= 1");
    if (misaligned(action_tape, 8)) return fail(HLX_ERR_INVALID, "hlx_eval_run: action_tape must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const size_t row = (size_t)ev->c.n_envs * HLX_ACT_DIM;
    auto act = [&](int64_t t) { return (action_tape && t < max_steps) ? action_tape + (size_t)t * row : ev->actions; };
    HIP_TRY(hipSetDevice(ev->c.device));
    int rc = hlx_reset(env, nullptr, ev->obs, stream);
    if (rc) return rc;
    rc = eval_begin(ev, ev->obs, act(0), s);
    if (rc) return rc;
    hlx_info_soa info;
    memset(&info, 0, sizeof info);
    info.packed = (float*)ev->packed;
    int64_t t = 0;
    while (t < max_steps) {
        rc = hlx_step(env, act(t), ev->obs, ev->reward, ev->term, ev->trunc, ev->terminal_obs, nullptr, nullptr, &info, stream);
        if (rc) return rc;
        EvalIo io{ev->obs, ev->reward, ev->term, ev->trunc, ev->terminal_obs, nullptr, nullptr, nullptr, ev->packed, act(t + 1)};
        rc = eval_observe(ev, io, s);
        if (rc) return rc;
        t += 1;
        if (steps_run) *steps_run = t;
        if (t % check_every == 0 || t == max_steps) {
            HIP_TRY(hipMemcpyAsync(ev->count_host, ev->k.count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (*ev->count_host >= ev->c.n_envs) break;
        }
    }
    return HLX_OK;
}

int hlx_eval_done_count(hlx_eval* ev, int32_t* out, void* stream) {
    if (!ev || !out) return fail(HLX_ERR_INVALID, "hlx_eval_done_count: null argument");
    HIP_TRY(hipSetDevice(ev->c.device));
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(ev->count_host, ev->k.count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = *ev->count_host;
    return HLX_OK;
}

int hlx_eval_records(hlx_eval* ev, float* min_distance, float* final_distance, int32_t* steps, float* total_reward, float* fuel_used,
                     int32_t* lock_losses, int32_t* lock_recoveries, uint8_t* success, int32_t* episodes, void* stream) {
    if (!ev) return fail(HLX_ERR_INVALID, "hlx_eval_records: null handle");
    HIP_TRY(hipSetDevice(ev->c.device));
    const hipStream_t s = (hipStream_t)stream;
    const size_t R = (size_t)ev->c.episodes_per_env * ev->c.n_envs;
    const struct { void* dst; const void* src; size_t bytes; } planes[] = {
        {min_distance, ev->k.r_mind, 4 * R}, {final_distance, ev->k.r_final, 4 * R}, {steps, ev->k.r_steps, 4 * R},
        {total_reward, ev->k.r_ret, 4 * R}, {fuel_used, ev->k.r_fuel, 4 * R}, {lock_losses, ev->k.r_loss, 4 * R},
        {lock_recoveries, ev->k.r_rec, 4 * R}, {success, ev->k.r_success, R}};
    for (const auto& p : planes)
        if (p.dst) HIP_TRY(hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToHost, s));
    if (episodes) {
        std::vector<int4> ai((size_t)ev->c.n_envs);
        HIP_TRY(hipMemcpyAsync(ai.data(), ev->k.acci, sizeof(int4) * ai.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (size_t i = 0; i < ai.size(); ++i) episodes[i] = ai[i].w >> 2;
    }
    HIP_TRY(hipStreamSynchronize(s));
    return HLX_OK;
}

}  // extern "C"
