// BranchingDQNPolicy's four small passes (tianshou/policy/modelfree/bdq.py, BranchingNet in
// utils/net/common.py:531-544): the dueling aggregation inside each branch with the greedy
// action per branch, its backward, the 1-step target with the mean over branches (:50-84) and
// learn()'s TD loss with its gradient and the outgoing priority (:113-126).  Q is [b, K, A]
// f32, row-major; a BDQ minibatch is 32 to a few hundred rows of K <= ~20 branches with
// A <= ~40 actions each, so the work is launch latency and each kernel replaces 4-15 torch
// launches.
//
// combine / target: one workgroup per batch row, wave w takes the branches w, w + 4, ...; its
// lanes run over the A actions (looping past 64).  Means and argmaxes are wave reductions, so
// no LDS row is staged and there is no width limit.
// td: one lane per batch row walks its K branches (as redq.hip walks ensemble members); the
// [rows, K, A] gradient tile is then written by the whole workgroup in storage order.
#include "loss_sum.h"

#pragma clang fp contract(off)

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;
constexpr int NW = TPB / kWave;

// torch's max over a row: the first index of the maximum, a NaN beats every number (the
// first NaN wins).  (v2, i2) replaces (v1, i1):
__device__ __forceinline__ bool better(float v2, int i2, float v1, int i1) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n2 && (!n1 || i2 < i1);
    return v2 > v1 || (v2 == v1 && i2 < i1);
}

// The wave's first-index argmax of (val, idx); lanes without an element hold (-inf, INT_MAX).
__device__ __forceinline__ int wave_argmax(float val, int idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float v2 = __shfl_xor(val, off, kWave);
        const int i2 = __shfl_xor(idx, off, kWave);
        if (better(v2, i2, val, idx)) {
            val = v2;
            idx = i2;
        }
    }
    return idx;
}

__device__ __forceinline__ int row_argmax(const float* __restrict__ x, int A, int lane) {
    float best = -INFINITY;
    int arg = INT_MAX;
    for (int a = lane; a < A; a += kWave) {
        const float v = x[a];
        if (better(v, a, best, arg)) {
            best = v;
            arg = a;
        }
    }
    return wave_argmax(best, arg);
}

__global__ __launch_bounds__(TPB) void combine_fwd_kernel(const float* __restrict__ s,
                                                          const float* __restrict__ v, int K,
                                                          int A, float* __restrict__ out,
                                                          int64_t* __restrict__ act_out) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = blockIdx.x;
    const double vr = (double)v[r];
    for (int k = wv; k < K; k += NW) {
        const int64_t o = (r * K + k) * A;
        double sum = 0.0;
        for (int a = lane; a < A; a += kWave) sum += (double)s[o + a];
        const double mean = wave_sum(sum) / (double)A;
        float best = -INFINITY;
        int arg = INT_MAX;
        for (int a = lane; a < A; a += kWave) {
            const float q = (float)(vr + ((double)s[o + a] - mean));
            out[o + a] = q;
            if (better(q, a, best, arg)) {
                best = q;
                arg = a;
            }
        }
        if (act_out) {
            arg = wave_argmax(best, arg);
            if (lane == 0) act_out[r * K + k] = arg;
        }
    }
}

__global__ __launch_bounds__(TPB) void combine_bwd_kernel(const float* __restrict__ g_out, int K,
                                                          int A, float* __restrict__ g_s,
                                                          float* __restrict__ g_v) {
    __shared__ double red[NW];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = blockIdx.x;
    double acc = 0.0;  // this wave's branches, in branch order
    for (int k = wv; k < K; k += NW) {
        const int64_t o = (r * K + k) * A;
        double sum = 0.0;
        for (int a = lane; a < A; a += kWave) sum += (double)g_out[o + a];
        sum = wave_sum(sum);
        acc += sum;
        const double mean = sum / (double)A;
        for (int a = lane; a < A; a += kWave) g_s[o + a] = (float)((double)g_out[o + a] - mean);
    }
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < NW; ++i) t += red[i];
        g_v[r] = (float)t;
    }
}

__global__ __launch_bounds__(TPB) void target_kernel(const float* __restrict__ q_sel,
                                                     const float* __restrict__ q_eval,
                                                     const double* __restrict__ rew,
                                                     const uint8_t* __restrict__ end,
                                                     double gamma, int K, int A,
                                                     float* __restrict__ out) {
    __shared__ double red[NW];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t r = blockIdx.x;
    double acc = 0.0;
    for (int k = wv; k < K; k += NW) {
        const int64_t o = (r * K + k) * A;
        const int arg = row_argmax(q_sel + o, A, lane);
        acc += (double)q_eval[o + arg];
    }
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < NW; ++i) t += red[i];
        const double m = t / (double)K;
        out[r] = (float)(rew[r] + gamma * m * (end[r] ? 0.0 : 1.0));
    }
}

// A branch's TD error and the gradient entry at its taken action are formed in f32 with
// tsrl_dqn_td_fwd_bwd's operations, and the row's mean of squares is rounded to f32 before the
// weight multiplies it, so K == 1 is that kernel bit for bit; the sums over branches and over
// the batch are f64.
__global__ __launch_bounds__(TPB) void td_fwd_bwd_kernel(
    const float* __restrict__ q, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ weight, int64_t b, int K, int A,
    float inv_bk, float* __restrict__ grad_q, float* __restrict__ prio,
    double* __restrict__ partials, MeanLosses<1> fin) {
    __shared__ uint8_t s_ok[TPB];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * TPB;
    const int nrows = (int)min((int64_t)TPB, b - r0);
    double term[1] = {0.0};
    uint8_t ok = 0;
    if (t < nrows) {
        const int64_t r = r0 + t;
        const int64_t* a_row = act + r * K;
        ok = 1;
        for (int k = 0; k < K; ++k) ok &= (uint8_t)(a_row[k] >= 0 && a_row[k] < A);
        if (ok) {
            const float ret = returns[r];
            double sq = 0.0, sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const float td = ret - q[(r * K + k) * A + a_row[k]];
                sq += (double)(td * td);
                sum += (double)td;
            }
            const float w = weight ? weight[r] : 1.0f;
            term[0] = (double)((float)(sq / (double)K) * w);
            prio[r] = (float)sum;
        } else {  // an action outside [0, A): NaN loss and priority, no gradient
            term[0] = (double)NAN;
            prio[r] = NAN;
        }
    }
    s_ok[t] = ok;
    double s[1];
    block_sums<1>(term, s);
    const int64_t ka = (int64_t)K * A;
    const int64_t nel = (int64_t)nrows * ka;
    const int64_t base = r0 * ka;
    for (int64_t f = t; f < nel; f += TPB) {
        const int row = (int)(f / ka);
        const int64_t rem = f - (int64_t)row * ka;
        const int k = (int)(rem / A);
        const int col = (int)(rem - (int64_t)k * A);
        float g = 0.0f;
        if (s_ok[row] && act[(r0 + row) * K + k] == col) {
            const float td = returns[r0 + row] - q[base + f];
            const float w = weight ? weight[r0 + row] : 1.0f;
            g = -2.0f * td * w * inv_bk;
        }
        grad_q[base + f] = g;
    }
    losses_or_partials<1>(s, partials, fin);
}

inline bool shape_ok(int64_t b, int64_t K, int64_t A) {
    return b >= 0 && b < ((int64_t)1 << 31) && K >= 1 && K < ((int64_t)1 << 31) && A >= 1 &&
           A < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_bdq_combine_fwd(const float* s, const float* v, int64_t b, int64_t K,
                                    int64_t A, float* out, int64_t* act_out, void* stream) {
    TSRL_CHECK_ARG(shape_ok(b, K, A), "tsrl_bdq_combine_fwd: need 0 <= b < 2^31, 1 <= K, A < 2^31");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(s && v && out, "tsrl_bdq_combine_fwd: null pointer");
    hipLaunchKernelGGL(combine_fwd_kernel, dim3((unsigned)b), dim3(TPB), 0, as_stream(stream), s,
                       v, (int)K, (int)A, out, act_out);
    TSRL_LAUNCH_CHECK("tsrl_bdq_combine_fwd");
    return 0;
}

extern "C" int tsrl_bdq_combine_bwd(const float* g_out, int64_t b, int64_t K, int64_t A,
                                    float* g_s, float* g_v, void* stream) {
    TSRL_CHECK_ARG(shape_ok(b, K, A), "tsrl_bdq_combine_bwd: need 0 <= b < 2^31, 1 <= K, A < 2^31");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(g_out && g_s && g_v, "tsrl_bdq_combine_bwd: null pointer");
    hipLaunchKernelGGL(combine_bwd_kernel, dim3((unsigned)b), dim3(TPB), 0, as_stream(stream),
                       g_out, (int)K, (int)A, g_s, g_v);
    TSRL_LAUNCH_CHECK("tsrl_bdq_combine_bwd");
    return 0;
}

extern "C" int tsrl_bdq_target(const float* q_sel, const float* q_eval, const double* rew,
                               const uint8_t* end, double gamma, int is_double, int64_t b,
                               int64_t K, int64_t A, float* out, void* stream) {
    TSRL_CHECK_ARG(shape_ok(b, K, A), "tsrl_bdq_target: need 0 <= b < 2^31, 1 <= K, A < 2^31");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(q_eval && rew && end && out && (!is_double || q_sel),
                   "tsrl_bdq_target: null pointer");
    hipLaunchKernelGGL(target_kernel, dim3((unsigned)b), dim3(TPB), 0, as_stream(stream),
                       is_double ? q_sel : q_eval, q_eval, rew, end, gamma, (int)K, (int)A, out);
    TSRL_LAUNCH_CHECK("tsrl_bdq_target");
    return 0;
}

extern "C" int tsrl_bdq_td_fwd_bwd(const float* q, const int64_t* act, const float* returns,
                                   const float* weight, int64_t b, int64_t K, int64_t A,
                                   float* grad_q, float* prio, double* partials, float* loss,
                                   void* stream) {
    TSRL_CHECK_ARG(b >= 1 && shape_ok(b, K, A),
                   "tsrl_bdq_td_fwd_bwd: need 1 <= b < 2^31, 1 <= K, A < 2^31");
    TSRL_CHECK_ARG(q && act && returns && grad_q && prio && loss,
                   "tsrl_bdq_td_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const MeanLosses<1> fin{(double)b, 1.0f, loss, nullptr};
    return launch_loss<1>("tsrl_bdq_td_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(td_fwd_bwd_kernel, dim3(nblk), dim3(TPB), 0, st, q, act, returns,
                           weight, b, (int)K, (int)A, 1.0f / ((float)b * (float)K), grad_q, prio,
                           partials, fin);
    });
}
