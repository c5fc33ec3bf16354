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
// work.  The batch sums are f64 in loss_sum.h's fixed order.  The temperature is read from
// device memory: it changes inside a replayed graph.
#include <cmath>

#include "loss_sum.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;  // one workgroup = 256 columns

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

// s[0] = sum_i sum_e(td[e, i]^2 * weight[i]), a column's E terms first, in index order.
__global__ __launch_bounds__(TPB) void redq_q_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ returns,
    const float* __restrict__ weight, int64_t E, int64_t b, float inv_n, float* __restrict__ gq,
    float* __restrict__ td_mean, double* __restrict__ partials, MeanLosses<1> fin) {
#pragma clang fp contract(off)
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
    block_sums<1>(term, s);
    losses_or_partials<1>(s, partials, fin);
}

// s[0] = sum_i(alpha * log_prob[i] - mean_e q[e, i]), s[1] = sum_i(log_prob[i] + target_entropy).
__global__ __launch_bounds__(TPB) void redq_actor_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ log_prob,
    const float* __restrict__ alpha, float target_entropy, int64_t E, int64_t b, float g_q,
    float inv_b, float* __restrict__ gq, float* __restrict__ g_logp,
    double* __restrict__ partials, ActorAlphaLosses fin) {
#pragma clang fp contract(off)
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
    block_sums<2>(term, s);
    losses_or_partials<2>(s, partials, fin);
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
    // 1 / (E b) rounded once; with E = 1 it is tsrl_q_mse_fwd_bwd's 1 / b
    const float inv_n = (float)(1.0 / ((double)E * (double)b));
    const hipStream_t st = as_stream(stream);
    const MeanLosses<1> fin{(double)E * (double)b, 1.0f, loss, nullptr};
    return launch_loss<1>("tsrl_redq_q_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(redq_q_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q, returns, weight,
                           E, b, inv_n, gq, td_mean, partials, fin);
    });
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
    const float g_q = (float)(-1.0 / ((double)E * (double)b));
    const hipStream_t st = as_stream(stream);
    const ActorAlphaLosses fin{(double)b, 1.0, log_alpha, loss, g_log_alpha};
    return launch_loss<2>("tsrl_redq_actor_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(redq_actor_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q, log_prob,
                           alpha, (float)target_entropy, E, b, g_q, 1.0f / (float)b, gq, g_logp,
                           partials, fin);
    });
}
