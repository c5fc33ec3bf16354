// REDQPolicy (tianshou/policy/modelfree/redq.py): the glue around the actor's and the critic
// ensemble's forwards.  REDQ runs many updates per environment step (20 in
// examples/mujoco/mujoco_redq.py), each a few launch-bound passes over an [E, b] block of Q
// values, E the ensemble size (10) and b the batch (256).
//   redq_target_kernel       _target_q's min / mean over the drawn subset of target critics,
//                            less alpha * log_prob (redq.py:150-155)
//   redq_q_loss_kernel       the ensemble's TD error, loss and gradient and the per-row mean TD
//                            error (redq.py:161-169)
//   redq_actor_loss_kernel   the actor loss on the ensemble mean, the temperature loss and every
//                            gradient of both (redq.py:176-189)
// q is [E, b] row-major, the critics' [E, b, 1] output: one lane owns column i and walks the E
// members, so every load is coalesced along i and a column's quantities need no cross-lane
// work.  The batch sums are f64 in the fixed order of ddpg.hip's q_mse_kernel.  The temperature
// is read from device memory: it changes inside a replayed graph.
#include <cmath>

#include "tsrl_common.h"

namespace tsrl {
namespace {

constexpr int TPB = 256;   // one workgroup = tsrl_ddpg_num_partials' 256 columns
constexpr int NW = TPB / kWave;

// torch.min: a NaN on either side is handed through.
__device__ __forceinline__ float min_nan(float a, float b) {
    return a != a ? a : (b != b ? b : (b < a ? b : a));
}

// The block's f64 sums: lanes by xor butterfly, the four waves in wave order.  Lane 0 returns
// the sums in s[0..nk).
template <int NK>
__device__ __forceinline__ void block_sums(const double* term, double (*red)[NW], double* s) {
    const int t = threadIdx.x;
    for (int k = 0; k < NK; ++k) {
        const double ws = wave_sum(term[k]);
        if ((t & (kWave - 1)) == 0) red[k][t / kWave] = ws;
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < NK; ++k) {
            s[k] = 0.0;
            for (int i = 0; i < NW; ++i) s[k] += red[k][i];
        }
    }
}

// mode 0: min over the subset; mode 1: its mean, summed in f64 in subset order.  The product and
// the difference are two f32 roundings (no FMA), as torch's `target_q -= alpha * log_prob`.  The
// host wrapper has validated the subset; an index outside [0, E) here reads nothing and gives NaN.
__global__ __launch_bounds__(TPB) void redq_target_kernel(
    const float* __restrict__ qs, int64_t E, int64_t b, const int32_t* __restrict__ idx,
    int64_t M, int mode, const float* __restrict__ log_prob, const float* __restrict__ alpha,
    float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= b) return;
    float mn = 0.0f;
    double sum = 0.0;
    for (int64_t m = 0; m < M; ++m) {
        const int64_t e = idx[m];
        const float v = (e >= 0 && e < E) ? qs[e * b + i] : NAN;
        mn = m == 0 ? v : min_nan(mn, v);
        sum += (double)v;
    }
    const float r = mode == 0 ? mn : (float)(sum / (double)M);
    const float p = alpha[0] * log_prob[i];
    out[i] = r - p;
}

__device__ __forceinline__ void finish_q_loss(double s, int64_t E, int64_t b, float* loss) {
    loss[0] = (float)(s / ((double)E * (double)b));
}

__global__ __launch_bounds__(TPB) void redq_q_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ returns,
    const float* __restrict__ weight, int64_t E, int64_t b, float inv_n, float* __restrict__ gq,
    float* __restrict__ td_mean, double* __restrict__ partials, float* __restrict__ loss) {
#pragma clang fp contract(off)
    __shared__ double red[1][NW];
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[1] = {0.0};
    if (i < b) {
        const float ret = returns[i];
        const float w = weight ? weight[i] : 1.0f;
        double tds = 0.0;
        for (int64_t e = 0; e < E; ++e) {
            const float td = q[e * b + i] - ret;
            term[0] += (double)(td * td * w);
            gq[e * b + i] = 2.0f * td * w * inv_n;
            tds += (double)td;
        }
        td_mean[i] = (float)(tds / (double)E);
    }
    double s[1];
    block_sums<1>(term, red, s);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1)
            finish_q_loss(s[0], E, b, loss);
        else
            partials[blockIdx.x] = s[0];
    }
}

__global__ void redq_q_fold_kernel(const double* __restrict__ partials, int64_t nblk, int64_t E,
                                   int64_t b, float* __restrict__ loss) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0.0;
        for (int64_t i = 0; i < nblk; ++i) s += partials[i];
        finish_q_loss(s, E, b, loss);
    }
}

// s[0] = sum_i(alpha * log_prob[i] - mean_e q[e, i]), s[1] = sum_i(log_prob[i] + target_entropy).
__device__ __forceinline__ void finish_actor_losses(const double* s, int64_t b,
                                                    const float* log_alpha, float* loss,
                                                    float* g_log_alpha) {
    loss[0] = (float)(s[0] / (double)b);
    if (log_alpha) {
        const double m = s[1] / (double)b;
        loss[1] = (float)(-(double)log_alpha[0] * m);
        g_log_alpha[0] = (float)(-m);
    }
}

__global__ __launch_bounds__(TPB) void redq_actor_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ log_prob,
    const float* __restrict__ alpha, const float* __restrict__ log_alpha, float target_entropy,
    int64_t E, int64_t b, float g_q, float inv_b, float* __restrict__ gq,
    float* __restrict__ g_logp, double* __restrict__ partials, float* __restrict__ loss,
    float* __restrict__ g_log_alpha) {
#pragma clang fp contract(off)
    __shared__ double red[2][NW];
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const float al = alpha[0];
    double term[2] = {0.0, 0.0};
    if (i < b) {
        const float lp = log_prob[i];
        double qs = 0.0;
        for (int64_t e = 0; e < E; ++e) {
            qs += (double)q[e * b + i];
            gq[e * b + i] = g_q;
        }
        const float p = al * lp;
        term[0] = (double)p - qs / (double)E;
        term[1] = (double)(lp + target_entropy);
        g_logp[i] = al * inv_b;
    }
    double s[2];
    block_sums<2>(term, red, s);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            finish_actor_losses(s, b, log_alpha, loss, g_log_alpha);
        } else {
            for (int k = 0; k < 2; ++k) partials[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
        }
    }
}

// partials [2][nblk] -> the losses and the temperature gradient.
__global__ void redq_actor_fold_kernel(const double* __restrict__ partials, int64_t nblk,
                                       int64_t b, const float* __restrict__ log_alpha,
                                       float* __restrict__ loss, float* __restrict__ g_log_alpha) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s[2] = {0.0, 0.0};
        for (int k = 0; k < 2; ++k)
            for (int64_t i = 0; i < nblk; ++i) s[k] += partials[(int64_t)k * nblk + i];
        finish_actor_losses(s, b, log_alpha, loss, g_log_alpha);
    }
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }
// b columns in one grid dimension, and E * b elements well inside int64
inline bool shape_ok(int64_t E, int64_t b) {
    return E >= 1 && E < ((int64_t)1 << 24) && b >= 1 && b < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_redq_target(const float* qs, int64_t E, int64_t b, const int32_t* idx,
                                const int32_t* idx_host, int64_t M, int mode,
                                const float* log_prob, const float* alpha, float* out,
                                void* stream) {
    TSRL_CHECK_ARG(shape_ok(E, b), "tsrl_redq_target: need E >= 1 and b >= 1");
    TSRL_CHECK_ARG(M >= 1 && M <= E, "tsrl_redq_target: need 1 <= M <= E (M %lld, E %lld)",
                   (long long)M, (long long)E);
    TSRL_CHECK_ARG(mode == 0 || mode == 1, "tsrl_redq_target: mode is 0 (min) or 1 (mean)");
    TSRL_CHECK_ARG(qs && idx && idx_host && log_prob && alpha && out,
                   "tsrl_redq_target: null pointer");
    for (int64_t m = 0; m < M; ++m)
        TSRL_CHECK_ARG(idx_host[m] >= 0 && idx_host[m] < E,
                       "tsrl_redq_target: idx[%lld] = %d is outside [0, %lld)", (long long)m,
                       (int)idx_host[m], (long long)E);
    hipLaunchKernelGGL(redq_target_kernel, dim3(blocks_of(b)), dim3(TPB), 0, as_stream(stream),
                       qs, E, b, idx, M, mode, log_prob, alpha, out);
    TSRL_LAUNCH_CHECK("tsrl_redq_target");
    return 0;
}

extern "C" int tsrl_redq_q_loss_fwd_bwd(const float* q, const float* returns,
                                        const float* weight, int64_t E, int64_t b, float* gq,
                                        float* td_mean, double* partials, float* loss,
                                        void* stream) {
    TSRL_CHECK_ARG(shape_ok(E, b), "tsrl_redq_q_loss_fwd_bwd: need E >= 1 and b >= 1");
    TSRL_CHECK_ARG(q && returns && gq && td_mean && loss,
                   "tsrl_redq_q_loss_fwd_bwd: null pointer");
    const int64_t nblk = tsrl_ddpg_num_partials(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "tsrl_redq_q_loss_fwd_bwd: b > %d needs partials",
                   TPB);
    // 1 / (E b) rounded once; with E = 1 it is tsrl_q_mse_fwd_bwd's 1 / b
    const float inv_n = (float)(1.0 / ((double)E * (double)b));
    hipLaunchKernelGGL(redq_q_loss_kernel, dim3((unsigned)nblk), dim3(TPB), 0,
                       as_stream(stream), q, returns, weight, E, b, inv_n, gq, td_mean, partials,
                       loss);
    TSRL_LAUNCH_CHECK("tsrl_redq_q_loss_fwd_bwd");
    if (nblk > 1) {
        hipLaunchKernelGGL(redq_q_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                           partials, nblk, E, b, loss);
        TSRL_LAUNCH_CHECK("tsrl_redq_q_loss_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_redq_actor_loss_fwd_bwd(const float* q, const float* log_prob,
                                            const float* alpha, const float* log_alpha,
                                            double target_entropy, int64_t E, int64_t b,
                                            float* gq, float* g_logp, double* partials,
                                            float* loss, float* g_log_alpha, void* stream) {
    TSRL_CHECK_ARG(shape_ok(E, b), "tsrl_redq_actor_loss_fwd_bwd: need E >= 1 and b >= 1");
    TSRL_CHECK_ARG(q && log_prob && alpha && gq && g_logp && loss,
                   "tsrl_redq_actor_loss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(!log_alpha || g_log_alpha,
                   "tsrl_redq_actor_loss_fwd_bwd: log_alpha needs g_log_alpha");
    const int64_t nblk = tsrl_ddpg_num_partials(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "tsrl_redq_actor_loss_fwd_bwd: b > %d needs partials",
                   TPB);
    const float g_q = (float)(-1.0 / ((double)E * (double)b));
    hipLaunchKernelGGL(redq_actor_loss_kernel, dim3((unsigned)nblk), dim3(TPB), 0,
                       as_stream(stream), q, log_prob, alpha, log_alpha, (float)target_entropy,
                       E, b, g_q, 1.0f / (float)b, gq, g_logp, partials, loss, g_log_alpha);
    TSRL_LAUNCH_CHECK("tsrl_redq_actor_loss_fwd_bwd");
    if (nblk > 1) {
        hipLaunchKernelGGL(redq_actor_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                           partials, nblk, b, log_alpha, loss, g_log_alpha);
        TSRL_LAUNCH_CHECK("tsrl_redq_actor_loss_fwd_bwd (fold)");
    }
    return 0;
}
