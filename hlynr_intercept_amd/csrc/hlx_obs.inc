// hlx_obs.inc -- on-device VecFrameStack + VecNormalize behind the step (C ABI: include/hlx_obs.h; included by
// hlx_kernels.hip after hlx_host.inc, whose error helpers it shares).
//
// Three small HBM-bound kernels per push (none of them re-shaped into anything else: this is byte moving plus a
// column reduction):
//   moments  : per-block partial sums / sums of squares (float64) of the N x (n_stack*D) stacked batch, read straight
//              from the raw frame ring with the zero-fill of young episodes applied on the fly; discounted returns.
//              Step pushes that follow a training push use the incremental form (newest frame only + corrections for the
//              environments that were reset: hlx_obs_moments_inc_kernel).
//   finalize : one block reduces the partials in a fixed order (deterministic, no float atomics), merges them into
//              the running mean/var/count with Chan's formula exactly as SB3's RunningMeanStd does, and refreshes
//              1/sqrt(var + eps).
//   emit     : the stacked batch, normalised and clipped, as 16-byte coalesced stores of [N][n_stack*D] float32;
//              terminal stacks of finished environments; normalised rewards; age bookkeeping.
// Algorithmic traffic per env and push at n_stack 4, D 26: frames 4 x 104 B read twice (moments + emit; the second
// read hits L2/MALL) + 416 B written.
#include <algorithm>

#include "../../include/hlx_obs.h"

namespace {

constexpr int OBS_MAX_STACK = 8;
constexpr int OBS_MOM_BLOCKS = 1024;

struct ObsK {
    const float* frames;      // [S][N][D] raw frame ring
    const uint8_t* age_in;    // frames since the episode's first observation, saturated at S-1
    uint8_t* age_out;
    const uint8_t* term;
    const uint8_t* trunc;
    int n, D, S, F;
    int slot_new;             // ring slot of the newest frame
    int mode;                 // 0 = step push, 1 = reset push (every age 0), 2 = re-emit (ages unchanged)
};

// term / trunc are never NULL here (the host substitutes an all-zero array): two unconditional byte loads, no
// short-circuit branch -- a branch per flag put a dependent load + wait per environment on the critical path
DEV bool obs_done(const ObsK& k, int i) {
    const unsigned d = (unsigned)k.term[i] | (unsigned)k.trunc[i];
    return k.mode == 0 && d != 0u;
}
DEV int obs_age(const ObsK& k, int i, bool done) {
    const int a = k.age_in[i];   // unconditional load; selects, no branches
    const int stepped = k.mode == 2 ? a : min(a + 1, k.S - 1);
    return (k.mode == 1 || done) ? 0 : stepped;
}
// element e of environment i's stack: position j = e / D (0 = oldest), feature f = e % D; zero while the episode
// is younger than the position is old (SB3 StackedObservations: the stack is zeroed at reset / on done)
DEV float obs_stacked(const ObsK& k, int i, int e, int age) {
    const int j = e / k.D, f = e - j * k.D, back = k.S - 1 - j;
    if (back > age) return 0.f;
    int slot = k.slot_new - back;
    if (slot < 0) slot += k.S;
    return k.frames[((size_t)slot * k.n + i) * k.D + f];
}

__global__ void hlx_obs_moments_kernel(ObsK k, const float* __restrict__ reward, double* __restrict__ returns,
                                       double gamma, double* __restrict__ partial, int R, int want_obs) {
    extern __shared__ double lds[];
    const int t = threadIdx.x, f = t % k.D, r = t / k.D;
    const int epb = (k.n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * epb, hi = min(k.n, lo + epb);
    double sum[OBS_MAX_STACK], sq[OBS_MAX_STACK];
#pragma unroll
    for (int j = 0; j < OBS_MAX_STACK; ++j) { sum[j] = 0.; sq[j] = 0.; }
    if (want_obs && r < R) {
#pragma unroll 2
        for (int i = lo + r; i < hi; i += R) {
            const int age = obs_age(k, i, obs_done(k, i));
            // every frame is loaded unconditionally (the ring is always initialised) and masked afterwards, so the
            // loads of consecutive iterations can be in flight together
            float v[OBS_MAX_STACK];
#pragma unroll
            for (int back = 0; back < OBS_MAX_STACK; ++back) {
                int slot = k.slot_new - back;
                if (slot < 0) slot += k.S;
                v[back] = back < k.S ? k.frames[((size_t)slot * k.n + i) * k.D + f] : 0.f;
            }
#pragma unroll
            for (int back = 0; back < OBS_MAX_STACK; ++back) {
                const double x = (back < k.S && back <= age) ? (double)v[back] : 0.0;
                sum[back] += x;      // indexed by age-of-frame here (a compile-time index), by position below
                sq[back] += x * x;
            }
        }
    }
    // discounted returns: VecNormalize._update_reward (returns = returns * gamma + reward), then their moments
    double rs = 0., rq = 0.;
    if (reward) {
        for (int i = lo + t; i < hi; i += blockDim.x) {
            const double ret = returns[i] * gamma + (double)reward[i];
            returns[i] = ret;
            rs += ret;
            rq += ret * ret;
        }
    }
    // block reduction in a fixed order
    double* mine = lds + (size_t)t * (2 * OBS_MAX_STACK + 2);
#pragma unroll
    for (int back = 0; back < OBS_MAX_STACK; ++back)
        if (back < k.S) { mine[2 * (k.S - 1 - back)] = sum[back]; mine[2 * (k.S - 1 - back) + 1] = sq[back]; }
    // returns: wave-level shuffle tree (fixed order); lane 0 of each wave holds the wave's sums
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { rs += __shfl_down(rs, off); rq += __shfl_down(rq, off); }
    mine[2 * OBS_MAX_STACK] = rs; mine[2 * OBS_MAX_STACK + 1] = rq;
    __syncthreads();
    double* out = partial + (size_t)blockIdx.x * (2 * k.F + 2);
    if (r == 0) {
        for (int j = 0; j < k.S; ++j) {
            double a = 0., b = 0.;
            for (int rr = 0; rr < R; ++rr) {
                const double* o = lds + (size_t)(rr * k.D + f) * (2 * OBS_MAX_STACK + 2);
                a += o[2 * j]; b += o[2 * j + 1];
            }
            out[2 * (j * k.D + f)] = a; out[2 * (j * k.D + f) + 1] = b;
        }
    }
    if (t == 0) {
        double a = 0., b = 0.;
        const int waves = ((int)blockDim.x + 63) >> 6;
        for (int w = 0; w < waves; ++w) {
            const double* o = lds + (size_t)(w * 64) * (2 * OBS_MAX_STACK + 2);
            a += o[2 * OBS_MAX_STACK]; b += o[2 * OBS_MAX_STACK + 1];
        }
        out[2 * k.F] = a; out[2 * k.F + 1] = b;
    }
}

// The same reduction for an even D (the intercept observation: 26): a thread owns a PAIR of adjacent features and reads
// them with one 8-byte load per frame (frame rows are D*4 bytes, so pairs stay 8-byte aligned), twice the bytes per
// load instruction and half the address arithmetic of the scalar form above.
template <int S>   // n_stack at compile time: with a run-time bound every frame load sat behind its own branch + wait
__global__ __launch_bounds__(256) void hlx_obs_moments_pair_kernel(ObsK k, const float* __restrict__ reward, double* __restrict__ returns,
                                                                   double gamma, double* __restrict__ partial, int R, int want_obs) {
    __shared__ double lds[256][4];
    __shared__ double rlds[4][2];
    const int H = k.D >> 1, t = threadIdx.x, m = t % H, r = t / H;
    const int epb = (k.n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * epb, hi = min(k.n, lo + epb);
    double s0[S], s1[S], q0[S], q1[S];
#pragma unroll
    for (int j = 0; j < S; ++j) { s0[j] = 0.; s1[j] = 0.; q0[j] = 0.; q1[j] = 0.; }
    if (want_obs && r < R) {
        const size_t plane = (size_t)k.n * k.D;
        const float* src[S];
#pragma unroll
        for (int back = 0; back < S; ++back) {
            int slot = k.slot_new - back;
            if (slot < 0) slot += S;
            src[back] = k.frames + (size_t)slot * plane + 2 * m;
        }
        constexpr int E = 4;   // environments per trip: E x S 8-byte loads in flight per lane
        for (int i0 = lo + r; i0 < hi; i0 += E * R) {
            float2 v[E][S];
            int age[E];
#pragma unroll
            for (int u = 0; u < E; ++u) {
                const int i = i0 + u * R, ii = i < hi ? i : lo;
                age[u] = i < hi ? obs_age(k, ii, obs_done(k, ii)) : -1;
#pragma unroll
                for (int back = 0; back < S; ++back)
                    v[u][back] = *reinterpret_cast<const float2*>(src[back] + (size_t)ii * k.D);
            }
#pragma unroll
            for (int u = 0; u < E; ++u) {
#pragma unroll
                for (int back = 0; back < S; ++back) {
                    const bool ok = back <= age[u];
                    const double x = ok ? (double)v[u][back].x : 0.0, y = ok ? (double)v[u][back].y : 0.0;
                    s0[back] += x; q0[back] += x * x; s1[back] += y; q1[back] += y * y;
                }
            }
        }
    }
    double rs = 0., rq = 0.;
    if (reward) {
        for (int i = lo + t; i < hi; i += blockDim.x) {
            const double ret = returns[i] * gamma + (double)reward[i];
            returns[i] = ret;
            rs += ret;
            rq += ret * ret;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { rs += __shfl_down(rs, off); rq += __shfl_down(rq, off); }
        if ((t & 63) == 0) { rlds[t >> 6][0] = rs; rlds[t >> 6][1] = rq; }
    }
    double* out = partial + (size_t)blockIdx.x * (2 * k.F + 2);
    // rows -> block sums, one stack position at a time (fixed order over the rows)
#pragma unroll
    for (int back = 0; back < S; ++back) {
        {
            __syncthreads();
            lds[t][0] = s0[back]; lds[t][1] = q0[back]; lds[t][2] = s1[back]; lds[t][3] = q1[back];
            __syncthreads();
            // 4 H outputs per position; for D > 128 the block (R H threads, R <= 3) has fewer threads than that
            for (int q = t; q < 4 * H; q += blockDim.x) {
                const int mm = q >> 2, w = q & 3;
                double a = 0.;
                for (int rr = 0; rr < R; ++rr) a += lds[rr * H + mm][w];
                const int col = (S - 1 - back) * k.D + 2 * mm + (w >> 1);   // w: 0 sum.x, 1 sq.x, 2 sum.y, 3 sq.y
                out[2 * col + (w & 1)] = a;
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        double a = 0., b = 0.;
        if (reward) {
            const int waves = ((int)blockDim.x + 63) >> 6;
            for (int w = 0; w < waves; ++w) { a += rlds[w][0]; b += rlds[w][1]; }
        }
        out[2 * k.F] = a; out[2 * k.F + 1] = b;
    }
}

// Incremental form of the same column sums for step pushes (mode 0) that follow a push whose sums are still at hand.
// Column block `back` (0 = newest frame) of the stacked batch at push t holds, for every environment that was not reset at
// t, exactly what block back-1 held at push t-1 (same frame, same zero-fill rule: age_t >= back <=> age_{t-1} >= back-1),
// and nothing for the environments that were (their stack is zeroed).  So
//     sum_back(t) = sum_{back-1}(t-1) - SUM over envs reset at t of [age_{t-1} >= back-1] * x_{t-back},   back >= 1,
// and only the NEWEST frame has to be read for all N environments (1/S of the traffic); the older frames are read for the
// few environments that finished this step.  This kernel writes, per block, the plain partial sums of the newest frame
// in its columns and the CORRECTION partial sums in the columns of the older positions; the finalize kernel subtracts
// them from the previous push's column sums.  Same fixed summation order as the full kernel, no atomics.
template <int S>
__global__ __launch_bounds__(256) void hlx_obs_moments_inc_kernel(ObsK k, const float* __restrict__ reward, double* __restrict__ returns,
                                                                  double gamma, double* __restrict__ partial, int R) {
    __shared__ double lds[256][4];
    __shared__ double rlds[4][2];
    const int H = k.D >> 1, t = threadIdx.x, m = t % H, r = t / H;
    const int epb = (k.n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * epb, hi = min(k.n, lo + epb);
    double s0[S], s1[S], q0[S], q1[S];      // [0]: newest frame; [b >= 1]: corrections of position b
#pragma unroll
    for (int j = 0; j < S; ++j) { s0[j] = 0.; s1[j] = 0.; q0[j] = 0.; q1[j] = 0.; }
    if (r < R) {
        const size_t plane = (size_t)k.n * k.D;
        const float* src[S];
#pragma unroll
        for (int back = 0; back < S; ++back) {
            int slot = k.slot_new - back;
            if (slot < 0) slot += S;
            src[back] = k.frames + (size_t)slot * plane + 2 * m;
        }
        constexpr int E = 8;   // environments per trip: E 8-byte loads in flight per lane
        for (int i0 = lo + r; i0 < hi; i0 += E * R) {
            float2 v[E];
            bool done[E];
#pragma unroll
            for (int u = 0; u < E; ++u) {
                const int i = i0 + u * R, ii = i < hi ? i : lo;
                v[u] = *reinterpret_cast<const float2*>(src[0] + (size_t)ii * k.D);
                done[u] = i < hi && obs_done(k, ii);
                if (i >= hi) v[u] = make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < E; ++u) {
                const double x = (double)v[u].x, y = (double)v[u].y;
                s0[0] += x; q0[0] += x * x; s1[0] += y; q1[0] += y * y;
                if (done[u]) {          // rare: this environment's older frames leave the batch
                    const int i = i0 + u * R, old_age = k.age_in[i];
#pragma unroll
                    for (int back = 1; back < S; ++back) {
                        if (back - 1 <= old_age) {
                            const float2 w = *reinterpret_cast<const float2*>(src[back] + (size_t)i * k.D);
                            const double a = (double)w.x, b = (double)w.y;
                            s0[back] += a; q0[back] += a * a; s1[back] += b; q1[back] += b * b;
                        }
                    }
                }
            }
        }
    }
    double rs = 0., rq = 0.;
    if (reward) {
        for (int i = lo + t; i < hi; i += blockDim.x) {
            const double ret = returns[i] * gamma + (double)reward[i];
            returns[i] = ret;
            rs += ret;
            rq += ret * ret;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { rs += __shfl_down(rs, off); rq += __shfl_down(rq, off); }
        if ((t & 63) == 0) { rlds[t >> 6][0] = rs; rlds[t >> 6][1] = rq; }
    }
    double* out = partial + (size_t)blockIdx.x * (2 * k.F + 2);
#pragma unroll
    for (int back = 0; back < S; ++back) {
        __syncthreads();
        lds[t][0] = s0[back]; lds[t][1] = q0[back]; lds[t][2] = s1[back]; lds[t][3] = q1[back];
        __syncthreads();
        for (int q = t; q < 4 * H; q += blockDim.x) {     // (as in hlx_obs_moments_pair_kernel: D > 128 loops)
            const int mm = q >> 2, w = q & 3;
            double a = 0.;
            for (int rr = 0; rr < R; ++rr) a += lds[rr * H + mm][w];
            const int col = (S - 1 - back) * k.D + 2 * mm + (w >> 1);
            out[2 * col + (w & 1)] = a;
        }
    }
    __syncthreads();
    if (t == 0) {
        double a = 0., b = 0.;
        if (reward) {
            const int waves = ((int)blockDim.x + 63) >> 6;
            for (int w = 0; w < waves; ++w) { a += rlds[w][0]; b += rlds[w][1]; }
        }
        out[2 * k.F] = a; out[2 * k.F + 1] = b;
    }
}

// stats layout (doubles): mean[F] | var[F] | inv_std[F] | -, ret_mean, ret_var, -, ret_inv_std, -, -, -   (counts: host)
// RunningMeanStd.update_from_moments (SB3 common/running_mean_std.py), float64 throughout
DEV void rms_merge(double& mean, double& var, double count, double bmean, double bvar, double bcount) {
    const double delta = bmean - mean, tot = count + bcount;
    const double new_mean = mean + delta * bcount / tot;
    const double m2 = var * count + bvar * bcount + (delta * delta) * count * bcount / (count + bcount);
    mean = new_mean;
    var = m2 / (count + bcount);
}

// One block per column (c < F: a feature of the stacked observation, c == F: the discounted returns): 256 threads
// add the B partials of that column in a fixed order (strided loads, LDS tree), thread 0 merges the result into
// the running statistics.  The sample counts are tracked by the host (they advance by n per training push), so
// the column blocks share nothing.
// colsum_prev / colsum_next: [F][2] batch sums (sum, sum of squares) of the previous / this push, kept for the incremental
// moments kernel; incremental != 0: the partials of the columns behind the newest frame are corrections to subtract from
// the previous push's sums of the position one step younger (see hlx_obs_moments_inc_kernel).
__global__ __launch_bounds__(256) void hlx_obs_finalize_kernel(const double* __restrict__ partial, int B, int F, int n,
                                                               double* __restrict__ stats, int merge_obs, int merge_ret, double eps,
                                                               double count, double rcount, const double* __restrict__ colsum_prev,
                                                               double* __restrict__ colsum_next, int D, int incremental) {
    __shared__ double red[256][2];
    const int c = blockIdx.x, t = threadIdx.x;
    const bool merge = (c < F) ? merge_obs != 0 : merge_ret != 0;
    double a = 0., b = 0.;
    if (merge) {
        for (int blk = t; blk < B; blk += 256) {
            const double* o = partial + (size_t)blk * (2 * F + 2) + 2 * c;
            a += o[0]; b += o[1];
        }
    }
    red[t][0] = a; red[t][1] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) { red[t][0] += red[t + w][0]; red[t][1] += red[t + w][1]; }
        __syncthreads();
    }
    if (t != 0) return;
    double* sc = stats + 3 * F;
    double tot = red[0][0], tot2 = red[0][1];
    if (c < F && merge) {
        if (incremental && c < F - D) {          // not the newest frame: stacked column c was column c + D one push ago
            tot = colsum_prev[2 * (c + D)] - tot;
            tot2 = colsum_prev[2 * (c + D) + 1] - tot2;
        }
        if (colsum_next) { colsum_next[2 * c] = tot; colsum_next[2 * c + 1] = tot2; }
    }
    const double bmean = tot / (double)n, bvar0 = tot2 / (double)n - bmean * bmean;   // population variance, as np.var
    const double bvar = bvar0 < 0. ? 0. : bvar0;
    if (c < F) {
        double m = stats[c], v = stats[F + c];
        if (merge) { rms_merge(m, v, count, bmean, bvar, (double)n); stats[c] = m; stats[F + c] = v; }
        stats[2 * F + c] = 1.0 / sqrt(v + eps);
    } else {
        double m = sc[1], v = sc[2];
        if (merge) { rms_merge(m, v, rcount, bmean, bvar, (double)n); sc[1] = m; sc[2] = v; }
        sc[4] = 1.0 / sqrt(v + eps);
    }
}

// The finalize kernel of a push whose NEWEST-frame column sums and return sums came out of the step kernel itself (hlx_obs_step
// -> KOpt::pipe_*: rows of `B` doubles, one entry per 64-environment block of the step launch).  One block per column of the
// stacked batch (+ one for the returns); what the incremental moments kernel used to contribute for the columns BEHIND the newest
// frame -- the rows of the environments that were reset in this step leave the batch -- is formed here from the blocks' done MASKS
// (one 64-bit ballot per block, left by the step kernel): for the few environments that finished, the frame value that leaves is
// added.  Fixed order, no atomics, no done list (whose order the launch does not define).
// Round 4 (7.2 -> see profiles/r04_obs_pipeline_*): the partials are stored transposed, so the 1 024 values of a column are four
// coalesced 8-byte loads per thread, all in flight at once (rows of 2 F + 4 doubles per block made each load a cache line of its
// own); the block's reduction is a DPP / shuffle tree inside each wave and one LDS hand-over between the four waves instead of
// eight __syncthreads() levels over LDS.
DEV void wave_sum2(double& a, double& b) {      // fixed-order butterfly-free tree: lane 0 ends up with lanes 0..63 added as ((0+32)+(16+48))+...
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
}
struct ObsFin {             // what finishing one push's statistics needs (hlx_obs_finalize_fused_kernel, or folded into the emit launch)
    const double* partial;  // [2 D + 3][B]
    int B, merge_ret;
    double eps, count, rcount;
    const double* colsum_prev;
    double* colsum_next;
};
DEV void obs_finalize_column(const ObsK& k, const ObsFin& fn, double* __restrict__ stats, int c, double (*red)[2]) {
    const double* __restrict__ partial = fn.partial;
    const int B = fn.B, merge_ret = fn.merge_ret;
    const double eps = fn.eps, count = fn.count, rcount = fn.rcount;
    const double* __restrict__ colsum_prev = fn.colsum_prev;
    double* __restrict__ colsum_next = fn.colsum_next;
    const int t = threadIdx.x, F = k.F, D = k.D, n = k.n;
    const bool newest = c >= F - D && c < F, ret_col = c == F;
    double a = 0., b = 0.;
    if (newest || (ret_col && merge_ret)) {
        const int row = ret_col ? 2 * D : 2 * (c - (F - D));
        const double* pa = partial + (size_t)row * B, *pb = pa + B;
        double va[4], vb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {            // B <= 1024 blocks: four loads per thread cover them (beyond that: the loop below)
            const int blk = t + 256 * j;
            va[j] = blk < B ? pa[blk] : 0.; vb[j] = blk < B ? pb[blk] : 0.;
        }
        a = (va[0] + va[1]) + (va[2] + va[3]); b = (vb[0] + vb[1]) + (vb[2] + vb[3]);
        for (int blk = t + 1024; blk < B; blk += 256) { a += pa[blk]; b += pb[blk]; }
    } else if (!ret_col) {
        // column c = position j (0 = oldest), feature f; it was column c + D one push ago.  Rows leaving: environments reset now whose
        // stack reached that far back (age_{t-1} >= back - 1)
        const int j = c / D, f = c - j * D, back = k.S - 1 - j;
        int slot = k.slot_new - back;
        if (slot < 0) slot += k.S;
        const float* src = k.frames + (size_t)slot * (size_t)n * D + f;
        // who finished: one 64-bit mask per block (row 2 D + 2, bit patterns); thread t takes blocks t, t + 256, ... and walks
        // their set bits in lane order
        const unsigned long long* masks = reinterpret_cast<const unsigned long long*>(partial + (size_t)(2 * D + 2) * B);
        for (int blk = t; blk < B; blk += 256) {
            unsigned long long m = masks[blk];
            while (m) {
                const int i = blk * 64 + __builtin_ctzll(m);
                m &= m - 1ull;
                const float xv = src[(size_t)i * D];          // (both loads at once: the age decides afterwards)
                const int ag = (int)k.age_in[i];
                const double x = (back - 1 <= ag) ? (double)xv : 0.0;
                a += x; b += x * x;
            }
        }
    }
    // what thread 0 needs for the merge is requested before the reduction (three dependent round trips behind it otherwise)
    double* sc = stats + 3 * F;
    double pm = 0., pv = 0., cp0 = 0., cp1 = 0.;
    if (t == 0) {
        if (!ret_col) { pm = stats[c]; pv = stats[F + c]; if (!newest) { cp0 = colsum_prev[2 * (c + D)]; cp1 = colsum_prev[2 * (c + D) + 1]; } }
        else { pm = sc[1]; pv = sc[2]; }
    }
    wave_sum2(a, b);
    if ((t & 63) == 0) { red[t >> 6][0] = a; red[t >> 6][1] = b; }
    __syncthreads();
    if (t == 0) {
    auto put = [](double* p, double v) { *p = v; };
    double tot = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]), tot2 = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    if (!ret_col) {
        if (!newest) { tot = cp0 - tot; tot2 = cp1 - tot2; }
        colsum_next[2 * c] = tot; colsum_next[2 * c + 1] = tot2;
    }
    const double bmean = tot / (double)n, bvar0 = tot2 / (double)n - bmean * bmean;
    const double bvar = bvar0 < 0. ? 0. : bvar0;
    if (!ret_col) {
        double m = pm, v = pv;
        rms_merge(m, v, count, bmean, bvar, (double)n);
        put(stats + c, m); put(stats + F + c, v);
        put(stats + 2 * F + c, 1.0 / sqrt(v + eps));
    } else {
        double m = pm, v = pv;
        if (merge_ret) { rms_merge(m, v, rcount, bmean, bvar, (double)n); put(sc + 1, m); put(sc + 2, v); }
        put(sc + 4, 1.0 / sqrt(v + eps));
    }
    }
}
__global__ __launch_bounds__(256) void hlx_obs_finalize_fused_kernel(ObsK k, ObsFin fn, double* __restrict__ stats) {
    __shared__ double red[4][2];
    obs_finalize_column(k, fn, stats, (int)blockIdx.x, red);
}

DEV float obs_norm(float raw, const double* stats, int F, int e, double clip) {
    // clip((obs - mean) / sqrt(var + eps)) in float64, cast to float32 (VecNormalize.normalize_obs); the division
    // is a multiplication by the float64 reciprocal computed once per push (<= 1 ulp(f64) away, gone after the cast)
    const double z = ((double)raw - stats[e]) * stats[2 * F + e];
    return (float)fmin(fmax(z, -clip), clip);
}

template <int PER>
__global__ __launch_bounds__(256) void hlx_obs_emit_kernel(ObsK k, const double* __restrict__ stats, int normalise, double clip_obs,
                                                           const float* __restrict__ terminal_obs, float* __restrict__ out,
                                                           float* __restrict__ term_out, const float* __restrict__ reward,
                                                           float* __restrict__ reward_out, int norm_reward, double clip_reward,
                                                           double* __restrict__ returns) {
    const int chunks = k.F / PER;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)k.n * chunks) return;
    const int i = (int)(idx / chunks), c = (int)(idx - (size_t)i * chunks);
    const bool done = obs_done(k, i);
    const int age = obs_age(k, i, done);
    float v[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int e = c * PER + q;
        const float raw = obs_stacked(k, i, e, age);
        v[q] = normalise ? obs_norm(raw, stats, k.F, e, clip_obs) : raw;
    }
    float* o = out + (size_t)i * k.F + c * PER;
    if (PER == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    else o[0] = v[0];
    if (done && term_out && terminal_obs) {
        // StackedObservations.update: terminal stack = (the stack before this step, shifted) + terminal observation
        const int age_prev = k.age_in[i];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int e = c * PER + q, j = e / k.D, f = e - j * k.D, back = k.S - 1 - j;
            float raw;
            if (back == 0) raw = terminal_obs[(size_t)i * k.D + f];
            else if (back - 1 > age_prev) raw = 0.f;
            else {
                int slot = k.slot_new - back;
                if (slot < 0) slot += k.S;
                raw = k.frames[((size_t)slot * k.n + i) * k.D + f];
            }
            v[q] = normalise ? obs_norm(raw, stats, k.F, e, clip_obs) : raw;
        }
        float* to = term_out + (size_t)i * k.F + c * PER;
        if (PER == 4) *reinterpret_cast<float4*>(to) = make_float4(v[0], v[1], v[2], v[3]);
        else to[0] = v[0];
    }
    if (c == 0) {
        if (k.mode != 2) k.age_out[i] = (uint8_t)age;
        if (reward && reward_out) {
            float r = reward[i];
            if (norm_reward) r = (float)fmin(fmax((double)r * stats[3 * k.F + 4], -clip_reward), clip_reward);
            reward_out[i] = r;
        }
        if (k.mode == 1 || done) returns[i] = 0.;   // VecNormalize.reset / step_wait: returns[dones] = 0
    }
}

// The emit pass for F % 4 == 0, even D and F/4 <= 256 (the intercept pipeline: 26 chunks): a thread owns ONE 16-byte
// chunk of the stacked row for a strip of environments, so the element -> (frame, feature) arithmetic, the four
// means and the four reciprocal deviations are computed once per thread and live in registers; per environment it
// issues two 8-byte frame loads and one 16-byte store.
// (Round 4 tried to finish the push's statistics INSIDE this launch -- the first F + 1 blocks reduce one column each, publish
// mean / var / 1/sqrt(var + eps) with device-scope stores and count themselves in; the other blocks issue their frame loads, wait
// for the count, then read their constants with device-scope loads.  Bit-identical, and slower: 35.4 against 28.7 us per training
// push (81.9 with acquire / release fences, which write back / invalidate a whole XCD's L2 per poll): a chain of device-scope
// round trips inside a launch is as long as the launch boundary it replaces.  profiles/r04_obs_pipeline_fold_negative.txt)
__global__ __launch_bounds__(256) void hlx_obs_emit_rows_kernel(ObsK k, const double* __restrict__ stats, int normalise, double clip_obs,
                                                                const float* __restrict__ terminal_obs, float* __restrict__ out,
                                                                float* __restrict__ term_out, const float* __restrict__ reward,
                                                                float* __restrict__ reward_out, int norm_reward, double clip_reward,
                                                                double* __restrict__ returns, int rows, int epb, uint32_t out_bytes) {
    const int chunks = k.F >> 2, c = threadIdx.x % chunks, r = threadIdx.x / chunks;
    if (r >= rows) return;
    // the stacked batch leaves through write-through (sc1) buffer stores, like the step's own outputs (hlx_kernels.hip):
    // the policy kernel that reads it is a later launch, and plain stores would wait dirty in L2 for the end-of-kernel
    // write-back.  out_bytes = 0 (batch >= 4 GiB: beyond a buffer descriptor's range) selects plain stores.
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, out_bytes, 0x00020000);
    const size_t plane = (size_t)k.n * k.D;
    // the chunk's two feature pairs (a pair never straddles two frames: D is even)
    const int e0 = 4 * c, j0 = e0 / k.D, e1 = e0 + 2, j1 = e1 / k.D;
    const int fa = e0 - j0 * k.D, fb = e1 - j1 * k.D, back_a = k.S - 1 - j0, back_b = k.S - 1 - j1;
    int slot_a = k.slot_new - back_a, slot_b = k.slot_new - back_b;
    if (slot_a < 0) slot_a += k.S;
    if (slot_b < 0) slot_b += k.S;
    const float* src_a = k.frames + (size_t)slot_a * plane + fa;
    const float* src_b = k.frames + (size_t)slot_b * plane + fb;
    const int lo = blockIdx.x * epb, hi = min(k.n, lo + epb);
    // all loads of the strip first (8 environments x two 8-byte loads in flight per lane), then compute and store:
    // with one environment per trip the pass ran at the latency of a single load per 1 KiB of wave traffic
    constexpr int E = 8;
    const float2 z = make_float2(0.f, 0.f);
    float2 a[E], b[E];
    int age[E];
    bool done[E];
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const int i = lo + r + u * rows;
        const int ii = i < hi ? i : lo;
        a[u] = *reinterpret_cast<const float2*>(src_a + (size_t)ii * k.D);
        b[u] = *reinterpret_cast<const float2*>(src_b + (size_t)ii * k.D);
        done[u] = obs_done(k, ii);
        age[u] = obs_age(k, ii, done[u]);
    }
    const double m0 = stats[e0], m1 = stats[e0 + 1], m2 = stats[e0 + 2], m3 = stats[e0 + 3];
    const double v0 = stats[2 * k.F + e0], v1 = stats[2 * k.F + e0 + 1], v2 = stats[2 * k.F + e0 + 2], v3 = stats[2 * k.F + e0 + 3];
    const double ret_inv = stats[3 * k.F + 4];
    auto norm1 = [&](float raw, double m, double iv) {
        return normalise ? (float)fmin(fmax(((double)raw - m) * iv, -clip_obs), clip_obs) : raw;
    };
    auto norm4 = [&](float2 a, float2 b) { return make_float4(norm1(a.x, m0, v0), norm1(a.y, m1, v1), norm1(b.x, m2, v2), norm1(b.y, m3, v3)); };
#pragma unroll
    for (int u = 0; u < E; ++u) {
        const int i = lo + r + u * rows;
        if (i < hi) {
            const float4 o4 = norm4(make_float2(back_a <= age[u] ? a[u].x : 0.f, back_a <= age[u] ? a[u].y : 0.f),
                                    make_float2(back_b <= age[u] ? b[u].x : 0.f, back_b <= age[u] ? b[u].y : 0.f));
            if (out_bytes) wt16(rs_out, (uint32_t)(((size_t)i * k.F + e0) * 4), 0u, o4);
            else *reinterpret_cast<float4*>(out + (size_t)i * k.F + e0) = o4;
            if (done[u] && term_out && terminal_obs) {
                // StackedObservations.update: terminal stack = (the stack before this step, shifted) + terminal observation
                const int age_prev = k.age_in[i];
                // (plain if/else on values: a ?: between `*ptr` and `a[u]` is an lvalue select, which takes the
                // arrays' addresses and sends the whole load batch through scratch memory)
                float2 ta = z, tb = z;
                if (back_a == 0) { const float* tp = terminal_obs + (size_t)i * k.D + fa; ta = make_float2(tp[0], tp[1]); }
                else if (back_a - 1 <= age_prev) ta = make_float2(a[u].x, a[u].y);
                if (back_b == 0) { const float* tp = terminal_obs + (size_t)i * k.D + fb; tb = make_float2(tp[0], tp[1]); }
                else if (back_b - 1 <= age_prev) tb = make_float2(b[u].x, b[u].y);
                *reinterpret_cast<float4*>(term_out + (size_t)i * k.F + e0) = norm4(ta, tb);
            }
            if (c == 0) {
                if (k.mode != 2) k.age_out[i] = (uint8_t)age[u];
                if (reward && reward_out) {
                    float rw = reward[i];
                    if (norm_reward) rw = (float)fmin(fmax((double)rw * ret_inv, -clip_reward), clip_reward);
                    reward_out[i] = rw;
                }
                if (k.mode == 1 || done[u]) returns[i] = 0.;   // VecNormalize.reset / step_wait: returns[dones] = 0
            }
        }
    }
}

}  // namespace

struct hlx_obs {
    hlx_obs_config c;
    int D, S, F, B, R;
    float* frames;
    uint8_t* age[2];
    uint8_t* zeros;      // [N] all-zero flags, stands in for a NULL terminated / truncated argument
    double* returns;
    double* stats;
    double* partial;
    double* partial_step;              // [2 D + 3][step blocks]: partial sums + done mask written by the step kernel itself (hlx_obs_step, fused form)
    int step_blocks;
    double* colsum[2];                 // [F][2] column sums of the last two training pushes (double-buffered by push parity)
    bool colsum_valid;
    unsigned long long colsum_push;    // the push whose column sums are in colsum[colsum_push & 1]
    unsigned long long pushes;
    double obs_count, ret_count;   // RunningMeanStd.count of the two statistics (advance by n_envs per training push)
    bool have_reset;
};

namespace {

// true when the next step push may take its newest-frame sums from the step kernel: everything the incremental moments kernel needs
// (obs_launch below), and an observation width the step kernel's tile has
bool obs_can_fuse(const hlx_obs* p, bool have_reward) {
    const bool upd_obs = p->c.training && p->c.norm_obs;
    return upd_obs && have_reward && p->D == HLX_OBS_DIM && p->S > 1 && p->colsum_valid && p->colsum_push + 1ull == p->pushes &&
           p->partial_step != nullptr && !getenv("HLX_OBS_FULL_MOMENTS") && !getenv("HLX_OBS_NO_FUSE");
}

int obs_launch(hlx_obs* p, int mode, const uint8_t* term, const uint8_t* trunc, const float* terminal_obs, const float* reward,
               float* stacked_out, float* term_out, float* reward_out, int normalise, hipStream_t s, bool fused = false) {
    const int cur = (int)(p->pushes & 1ull);
    ObsK k;
    k.frames = p->frames; k.age_in = p->age[cur]; k.age_out = p->age[cur ^ 1]; k.term = term ? term : p->zeros; k.trunc = trunc ? trunc : p->zeros;
    k.n = p->c.n_envs; k.D = p->D; k.S = p->S; k.F = p->F; k.mode = mode;
    k.slot_new = (int)((mode == 2 ? p->pushes + (unsigned long long)p->S - 1ull : p->pushes) % (unsigned long long)p->S);
    const bool upd_obs = mode != 2 && p->c.training && p->c.norm_obs;
    const bool upd_ret = mode == 0 && p->c.training && reward != nullptr;
    if (fused) {
        // the step kernel has left this push's newest-frame and return sums in partial_step (hlx_obs_step): one launch finishes them
        ObsFin fn{};
        fn.partial = p->partial_step; fn.B = p->step_blocks; fn.merge_ret = 1; fn.eps = p->c.epsilon; fn.count = p->obs_count;
        fn.rcount = p->ret_count; fn.colsum_prev = p->colsum[(p->pushes + 1ull) & 1ull]; fn.colsum_next = p->colsum[p->pushes & 1ull];
        hipLaunchKernelGGL(hlx_obs_finalize_fused_kernel, dim3(p->F + 1), dim3(256), 0, s, k, fn, p->stats);
        HIP_TRY(hipGetLastError());
        p->colsum_valid = true; p->colsum_push = p->pushes;
        p->obs_count += (double)p->c.n_envs;
        p->ret_count += (double)p->c.n_envs;
    } else if (upd_obs || upd_ret) {
        // column sums of this push -> colsum[pushes & 1]; the incremental kernel needs those of the push before
        const bool pair_ok = (p->D & 1) == 0 && p->D <= 512;
        const bool inc = pair_ok && upd_obs && mode == 0 && p->S > 1 && p->colsum_valid && p->colsum_push + 1ull == p->pushes &&
                         !getenv("HLX_OBS_FULL_MOMENTS");
        const double* cs_prev = inc ? p->colsum[(p->pushes + 1ull) & 1ull] : nullptr;
        double* cs_next = (upd_obs && mode != 2) ? p->colsum[p->pushes & 1ull] : nullptr;
        if (inc) {
            const int H = p->D / 2, R = std::max(1, 256 / H);
#define HLX_MOM(SS)                                                                                                     \
    case SS:                                                                                                            \
        hipLaunchKernelGGL(hlx_obs_moments_inc_kernel<SS>, dim3(p->B), dim3(R * H), 0, s, k, upd_ret ? reward : nullptr, \
                           p->returns, p->c.gamma, p->partial, R);                                                      \
        break;
            switch (p->S) { HLX_MOM(2) HLX_MOM(3) HLX_MOM(4) HLX_MOM(5) HLX_MOM(6) HLX_MOM(7) HLX_MOM(8) }
#undef HLX_MOM
        } else if (pair_ok) {
            const int H = p->D / 2, R = std::max(1, 256 / H);
#define HLX_MOM(SS)                                                                                                     \
    case SS:                                                                                                            \
        hipLaunchKernelGGL(hlx_obs_moments_pair_kernel<SS>, dim3(p->B), dim3(R * H), 0, s, k, upd_ret ? reward : nullptr, \
                           p->returns, p->c.gamma, p->partial, R, upd_obs ? 1 : 0);                                     \
        break;
            switch (p->S) { HLX_MOM(1) HLX_MOM(2) HLX_MOM(3) HLX_MOM(4) HLX_MOM(5) HLX_MOM(6) HLX_MOM(7) HLX_MOM(8) }
#undef HLX_MOM
        } else {
            const int threads = p->R * p->D;
            const size_t lds = sizeof(double) * (size_t)threads * (2 * OBS_MAX_STACK + 2);
            hipLaunchKernelGGL(hlx_obs_moments_kernel, dim3(p->B), dim3(threads), lds, s, k, upd_ret ? reward : nullptr, p->returns,
                               p->c.gamma, p->partial, p->R, upd_obs ? 1 : 0);
        }
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hlx_obs_finalize_kernel, dim3(p->F + 1), dim3(256), 0, s, p->partial, p->B, p->F, p->c.n_envs, p->stats,
                           upd_obs ? 1 : 0, upd_ret ? 1 : 0, p->c.epsilon, p->obs_count, p->ret_count, cs_prev, cs_next, p->D, inc ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (cs_next) { p->colsum_valid = true; p->colsum_push = p->pushes; }
        if (upd_obs) p->obs_count += (double)p->c.n_envs;
        if (upd_ret) p->ret_count += (double)p->c.n_envs;
    }
    if (p->F % 4 == 0 && (p->D & 1) == 0 && p->F / 4 <= 256) {
        const int chunks = p->F / 4, rows = 256 / chunks, epb = rows * 8;   // 8 environments per thread
        const unsigned long long total = (unsigned long long)p->c.n_envs * p->F * 4ull;
        const uint32_t out_bytes = total < 0xFFFFFFFFull ? (uint32_t)total : 0u;
        hipLaunchKernelGGL(hlx_obs_emit_rows_kernel, dim3((unsigned)((p->c.n_envs + epb - 1) / epb)), dim3(256), 0, s, k, p->stats, normalise,
                           p->c.clip_obs, terminal_obs, stacked_out, term_out, reward, reward_out, p->c.norm_reward, p->c.clip_reward,
                           p->returns, rows, epb, out_bytes);
        HIP_TRY(hipGetLastError());
        if (mode != 2) p->pushes += 1;
        return HLX_OK;
    }
    const int per = (p->F % 4 == 0) ? 4 : 1;
    const size_t work = (size_t)p->c.n_envs * (p->F / per);
    const dim3 grid((unsigned)((work + 255) / 256));
    if (per == 4)
        hipLaunchKernelGGL(hlx_obs_emit_kernel<4>, grid, dim3(256), 0, s, k, p->stats, normalise, p->c.clip_obs, terminal_obs, stacked_out,
                           term_out, reward, reward_out, p->c.norm_reward, p->c.clip_reward, p->returns);
    else
        hipLaunchKernelGGL(hlx_obs_emit_kernel<1>, grid, dim3(256), 0, s, k, p->stats, normalise, p->c.clip_obs, terminal_obs, stacked_out,
                           term_out, reward, reward_out, p->c.norm_reward, p->c.clip_reward, p->returns);
    HIP_TRY(hipGetLastError());
    if (mode != 2) p->pushes += 1;
    return HLX_OK;
}

int obs_refresh(hlx_obs* p, hipStream_t s) {   // inv_std from the current mean/var (after set_stats / at creation)
    hipLaunchKernelGGL(hlx_obs_finalize_kernel, dim3(p->F + 1), dim3(256), 0, s, p->partial, p->B, p->F, p->c.n_envs, p->stats, 0, 0,
                       p->c.epsilon, p->obs_count, p->ret_count, (const double*)nullptr, (double*)nullptr, p->D, 0);
    HIP_TRY(hipGetLastError());
    return HLX_OK;
}

}  // namespace

extern "C" {

int hlx_obs_destroy(hlx_obs* p) {
    if (!p) return HLX_OK;
    (void)hipSetDevice(p->c.device);
    (void)hipDeviceSynchronize();
    if (p->frames) (void)hipFree(p->frames);
    if (p->age[0]) (void)hipFree(p->age[0]);
    if (p->returns) (void)hipFree(p->returns);
    if (p->stats) (void)hipFree(p->stats);
    if (p->partial) (void)hipFree(p->partial);
    if (p->partial_step) (void)hipFree(p->partial_step);
    if (p->colsum[0]) (void)hipFree(p->colsum[0]);
    delete p;
    return HLX_OK;
}

int hlx_obs_create(const hlx_obs_config* cfg, hlx_obs** out) {
    if (!cfg || !out) return fail(HLX_ERR_INVALID, "hlx_obs_create: null argument");
    if (cfg->n_envs < 1 || cfg->obs_dim < 1 || cfg->obs_dim > 256 || cfg->n_stack < 1 || cfg->n_stack > OBS_MAX_STACK)
        return fail(HLX_ERR_INVALID, "hlx_obs_create: need n_envs >= 1, 1 <= obs_dim <= 256, 1 <= n_stack <= %d", OBS_MAX_STACK);
    if (!(cfg->epsilon > 0.0) || !(cfg->clip_obs > 0.0) || !(cfg->clip_reward > 0.0))
        return fail(HLX_ERR_INVALID, "hlx_obs_create: epsilon, clip_obs and clip_reward must be positive");
    HIP_TRY(hipSetDevice(cfg->device));
    hlx_obs* p = new (std::nothrow) hlx_obs();
    if (!p) return fail(HLX_ERR_NOMEM, "hlx_obs_create: out of host memory");
    p->c = *cfg;
    p->D = cfg->obs_dim; p->S = cfg->n_stack; p->F = p->D * p->S;
    p->R = std::max(1, 256 / p->D);
    p->B = std::max(1, std::min(OBS_MOM_BLOCKS, (cfg->n_envs + 63) / 64));
    p->pushes = 0; p->have_reset = false; p->obs_count = 1e-4; p->ret_count = 1e-4;
    const size_t N = (size_t)cfg->n_envs;
    hipError_t err = hipMalloc(&p->frames, sizeof(float) * N * p->F);
    if (err == hipSuccess) err = hipMalloc(&p->age[0], 3 * N);
    if (err == hipSuccess) err = hipMalloc(&p->returns, sizeof(double) * N);
    if (err == hipSuccess) err = hipMalloc(&p->stats, sizeof(double) * (3 * p->F + 8));
    if (err == hipSuccess) err = hipMalloc(&p->partial, sizeof(double) * (size_t)p->B * (2 * p->F + 2));
    if (err == hipSuccess) err = hipMalloc(&p->colsum[0], sizeof(double) * 4 * (size_t)p->F);
    p->step_blocks = (cfg->n_envs + 63) / 64;
    if (err == hipSuccess) err = hipMalloc(&p->partial_step, sizeof(double) * (size_t)p->step_blocks * (2 * p->D + 3));
    if (err == hipSuccess) err = hipMemset(p->partial_step, 0, sizeof(double) * (size_t)p->step_blocks * (2 * p->D + 3));
    if (err != hipSuccess) {
        int rc = fail(err == hipErrorOutOfMemory ? HLX_ERR_NOMEM : HLX_ERR_HIP, "hlx_obs_create: hipMalloc: %s", hipGetErrorString(err));
        hlx_obs_destroy(p);
        return rc;
    }
    p->age[1] = p->age[0] + N; p->zeros = p->age[0] + 2 * N;
    p->colsum[1] = p->colsum[0] + 2 * (size_t)p->F; p->colsum_valid = false; p->colsum_push = 0;
    // RunningMeanStd(): mean 0, var 1, count 1e-4
    std::vector<double> h(3 * p->F + 8, 0.0);
    for (int e = 0; e < p->F; ++e) h[p->F + e] = 1.0;
    h[3 * p->F + 2] = 1.0;
    err = hipMemcpy(p->stats, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(p->frames, 0, sizeof(float) * N * p->F);
    if (err == hipSuccess) err = hipMemset(p->age[0], 0, 3 * N);
    if (err == hipSuccess) err = hipMemset(p->returns, 0, sizeof(double) * N);
    int rc = HLX_OK;
    if (err != hipSuccess) rc = fail(HLX_ERR_HIP, "hlx_obs_create: initialisation: %s", hipGetErrorString(err));
    if (rc == HLX_OK) rc = obs_refresh(p, nullptr);
    if (rc == HLX_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(HLX_ERR_HIP, "hlx_obs_create: synchronise failed");
    if (rc != HLX_OK) { hlx_obs_destroy(p); return rc; }
    *out = p;
    return HLX_OK;
}

float* hlx_obs_next_slot(hlx_obs* p) {
    if (!p) return nullptr;
    return p->frames + (size_t)(p->pushes % (unsigned long long)p->S) * (size_t)p->c.n_envs * p->D;
}

int32_t hlx_obs_feature_dim(const hlx_obs* p) { return p ? p->F : 0; }

int hlx_obs_push_reset(hlx_obs* p, float* stacked_out, void* stream) {
    if (!p || !stacked_out) return fail(HLX_ERR_INVALID, "hlx_obs_push_reset: null argument");
    HIP_TRY(hipSetDevice(p->c.device));
    p->have_reset = true;
    return obs_launch(p, 1, nullptr, nullptr, nullptr, nullptr, stacked_out, nullptr, nullptr, p->c.norm_obs, (hipStream_t)stream);
}

int hlx_obs_push(hlx_obs* p, const uint8_t* terminated, const uint8_t* truncated, const float* terminal_obs, const float* reward,
                 float* stacked_out, float* terminal_stacked_out, float* reward_out, void* stream) {
    if (!p || !stacked_out) return fail(HLX_ERR_INVALID, "hlx_obs_push: null argument");
    if (!p->have_reset) return fail(HLX_ERR_STATE, "hlx_obs_push: call hlx_obs_push_reset first");
    HIP_TRY(hipSetDevice(p->c.device));
    return obs_launch(p, 0, terminated, truncated, terminal_obs, reward, stacked_out, terminal_stacked_out, reward_out, p->c.norm_obs,
                      (hipStream_t)stream);
}

int hlx_obs_step(hlx_obs* p, hlx_env* env, const float* actions, float* reward, uint8_t* terminated, uint8_t* truncated,
                 float* terminal_obs, int32_t* done_idx, int32_t* n_done, const hlx_info_soa* info, float* stacked_out,
                 float* terminal_stacked_out, float* reward_out, void* stream) {
    if (!p || !env || !stacked_out) return fail(HLX_ERR_INVALID, "hlx_obs_step: null argument");
    if (!p->have_reset) return fail(HLX_ERR_STATE, "hlx_obs_step: call hlx_reset + hlx_obs_push_reset first");
    if (hlx_num_envs(env) != p->c.n_envs || p->D != HLX_OBS_DIM)
        return fail(HLX_ERR_INVALID, "hlx_obs_step: the pipeline was created for %d x %d observations, the environment set has %d x %d",
                    p->c.n_envs, p->D, hlx_num_envs(env), HLX_OBS_DIM);
    // Training pushes that can be incremental take the newest frame's column sums and the return sums from the step kernel
    // itself (KOpt::pipe_*): the moments pass over the batch disappears, one finalize launch and the emit remain.
    const bool fused = reward != nullptr && obs_can_fuse(p, true) && !env->step_noise && !env->reset_noise;
    if (fused) {
        env->pipe_partial = p->partial_step; env->pipe_returns = p->returns; env->pipe_gamma = p->c.gamma;
        env->pipe_stride = p->step_blocks; env->pipe_col0 = (p->S - 1) * p->D;     // rows of `step_blocks` doubles (KOpt::pipe_partial)
    }
    int rc = hlx_step(env, actions, hlx_obs_next_slot(p), reward, terminated, truncated, terminal_obs, done_idx, n_done, info, stream);
    env->pipe_partial = env->pipe_returns = nullptr;
    if (rc) return rc;
    return obs_launch(p, 0, terminated, truncated, terminal_obs, reward, stacked_out, terminal_stacked_out, reward_out, p->c.norm_obs,
                      (hipStream_t)stream, fused);
}

int hlx_obs_emit(hlx_obs* p, int32_t normalise, float* stacked_out, void* stream) {
    if (!p || !stacked_out) return fail(HLX_ERR_INVALID, "hlx_obs_emit: null argument");
    if (!p->have_reset) return fail(HLX_ERR_STATE, "hlx_obs_emit: nothing pushed yet");
    HIP_TRY(hipSetDevice(p->c.device));
    return obs_launch(p, 2, nullptr, nullptr, nullptr, nullptr, stacked_out, nullptr, nullptr, normalise ? 1 : 0, (hipStream_t)stream);
}

int hlx_obs_set_mode(hlx_obs* p, int32_t training, int32_t norm_obs, int32_t norm_reward) {
    if (!p) return fail(HLX_ERR_INVALID, "hlx_obs_set_mode: null handle");
    p->c.training = training != 0; p->c.norm_obs = norm_obs != 0; p->c.norm_reward = norm_reward != 0;
    return HLX_OK;
}

int hlx_obs_get_stats(hlx_obs* p, double* obs_mean, double* obs_var, double scalars[4]) {
    if (!p || !obs_mean || !obs_var || !scalars) return fail(HLX_ERR_INVALID, "hlx_obs_get_stats: null argument");
    HIP_TRY(hipSetDevice(p->c.device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> h(3 * p->F + 8);
    HIP_TRY(hipMemcpy(h.data(), p->stats, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
    memcpy(obs_mean, h.data(), sizeof(double) * p->F);
    memcpy(obs_var, h.data() + p->F, sizeof(double) * p->F);
    scalars[0] = p->obs_count; scalars[1] = h[3 * p->F + 1]; scalars[2] = h[3 * p->F + 2]; scalars[3] = p->ret_count;
    return HLX_OK;
}

int hlx_obs_set_stats(hlx_obs* p, const double* obs_mean, const double* obs_var, const double scalars[4]) {
    if (!p || !obs_mean || !obs_var || !scalars) return fail(HLX_ERR_INVALID, "hlx_obs_set_stats: null argument");
    HIP_TRY(hipSetDevice(p->c.device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> h(3 * p->F + 8, 0.0);
    memcpy(h.data(), obs_mean, sizeof(double) * p->F);
    memcpy(h.data() + p->F, obs_var, sizeof(double) * p->F);
    h[3 * p->F + 1] = scalars[1]; h[3 * p->F + 2] = scalars[2];
    p->obs_count = scalars[0]; p->ret_count = scalars[3];
    HIP_TRY(hipMemcpy(p->stats, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
    int rc = obs_refresh(p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return HLX_OK;
}

}  // extern "C"
