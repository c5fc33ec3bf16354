// SACPolicy (tianshou/policy/modelfree/sac.py): the glue around the actor and critic forwards.
// In torch the reparameterised tanh-Gaussian sample with its log-probability is about fifteen
// launches over a few hundred rows, taken twice per update and once per collector step, and
// Normal's argument validation adds a host sync each time: launch latency, as in ddpg.hip.
//   sac_sample_fwd_kernel   forward's rsample, tanh squashing and corrected log_prob
//                           (sac.py:117-128)
//   sac_sample_bwd_kernel   its analytic gradient towards mu and sigma
//   sac_target_kernel       _target_q's min(Q1, Q2) - alpha * log_prob (sac.py:141-144)
//   sac_actor_loss_kernel   the actor loss, the temperature loss and every gradient of both
//                           (sac.py:162-165, 171-173), summed in loss_sum.h's order
// The temperature is read from device memory in every kernel: it changes inside a replayed graph.
#include "loss_sum.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;
constexpr int RPB = 64;    // the sample forward: one row per lane, one wave per workgroup
constexpr float kEps32 = 0x1p-23f;                  // np.finfo(np.float32).eps
constexpr float kLogSqrt2Pi = 0.91893853320467274f;  // math.log(math.sqrt(2 * math.pi))

// One lane = one row: its A terms are summed in f64 in index order.  Every term is the f32
// expression torch evaluates (Normal.log_prob, then log((1 - act^2) + eps32)), no FMA.
__global__ __launch_bounds__(RPB) void sac_sample_fwd_kernel(
    const float* __restrict__ mu, const float* __restrict__ sigma, const float* __restrict__ eps,
    int64_t b, int64_t A, float* __restrict__ act, float* __restrict__ log_prob) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x;
    if (r >= b) return;
    double gauss = 0.0, corr = 0.0;
    for (int64_t j = 0; j < A; ++j) {
        const int64_t i = r * A + j;
        const float m = mu[i];
        const float s = sigma[i];
        float u = m;
        if (eps) {
            const float e = eps[i] * s;
            u = m + e;
        }
        const float a = tanhf(u);
        act[i] = a;
        const float d = u - m;
        const float var = s * s;
        const float t = -(d * d) / (2.0f * var) - logf(s) - kLogSqrt2Pi;
        gauss += (double)t;
        const float one_m = 1.0f - a * a;
        corr += (double)logf(one_m + kEps32);
    }
    log_prob[r] = (float)(gauss - corr);
}

// One lane = one element.  c = 2 act (1 - act^2) / ((1 - act^2) + eps32) is d(-log(1 - act^2 +
// eps32)) / du; a saturated action (1 - act^2 == 0) gives exactly 0.
__global__ __launch_bounds__(TPB) void sac_sample_bwd_kernel(
    const float* __restrict__ sigma, const float* __restrict__ eps, const float* __restrict__ act,
    const float* __restrict__ g_act, const float* __restrict__ g_logp, int64_t n, int64_t A,
    float* __restrict__ g_mu, float* __restrict__ g_sigma) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const float a = act[i];
    const float one_m = 1.0f - a * a;
    const float gl = g_logp ? g_logp[i / A] : 0.0f;
    float gm = g_act ? g_act[i] * one_m : 0.0f;
    if (g_logp) {
        const float c = 2.0f * a * one_m / (one_m + kEps32);
        gm = gm + gl * c;
    }
    g_mu[i] = gm;
    float gs = eps ? eps[i] * gm : 0.0f;
    if (g_logp) gs = gs - gl / sigma[i];
    g_sigma[i] = gs;
}

__global__ __launch_bounds__(TPB) void sac_target_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ log_prob,
    const float* __restrict__ alpha, int64_t b, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    const float p = alpha[0] * log_prob[r];
    out[r] = min_nan(q1[r], q2[r]) - p;
}

// One workgroup = 256 rows: s[0] = sum(alpha * log_prob - min(q1, q2)), s[1] = sum(log_prob +
// target_entropy), in loss_sum.h's fixed order.
__global__ __launch_bounds__(TPB) void sac_actor_loss_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ log_prob,
    const float* __restrict__ alpha, float target_entropy, int64_t b, float inv_b,
    float* __restrict__ g_q1, float* __restrict__ g_q2, float* __restrict__ g_logp,
    double* __restrict__ partials, ActorAlphaLosses fin) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const float al = alpha[0];
    double term[2] = {0.0, 0.0};
    if (r < b) {
        const float a = q1[r], c = q2[r], lp = log_prob[r];
        const float p = al * lp;
        term[0] = (double)(p - min_nan(a, c));
        term[1] = (double)(lp + target_entropy);
        // torch's minimum backward: where(self == other, grad / 2, grad), then zero where the
        // other side is smaller
        const float g = -inv_b;
        const float gt = a == c ? g / 2.0f : g;
        g_q1[r] = a > c ? 0.0f : gt;
        g_q2[r] = a < c ? 0.0f : gt;
        g_logp[r] = al * inv_b;
    }
    double s[2];
    block_sums<2>(term, s);
    losses_or_partials<2>(s, partials, fin);
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_sac_sample_fwd(const float* mu, const float* sigma, const float* eps,
                                   int64_t b, int64_t A, float* act, float* log_prob,
                                   void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * RPB, "tsrl_sac_sample_fwd: need b >= 1");
    TSRL_CHECK_ARG(A >= 1 && A < ((int64_t)1 << 24), "tsrl_sac_sample_fwd: need A >= 1");
    TSRL_CHECK_ARG(mu && sigma && act && log_prob, "tsrl_sac_sample_fwd: null pointer");
    hipLaunchKernelGGL(sac_sample_fwd_kernel, dim3(blocks_of(b, RPB)), dim3(RPB), 0,
                       as_stream(stream), mu, sigma, eps, b, A, act, log_prob);
    TSRL_LAUNCH_CHECK("tsrl_sac_sample_fwd");
    return 0;
}

extern "C" int tsrl_sac_sample_bwd(const float* sigma, const float* eps, const float* act,
                                   const float* g_act, const float* g_logp, int64_t b, int64_t A,
                                   float* g_mu, float* g_sigma, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && A >= 1 && A < ((int64_t)1 << 31) &&
                       b < ((int64_t)1 << 31) * TPB / A,
                   "tsrl_sac_sample_bwd: need b >= 1 and A >= 1");
    TSRL_CHECK_ARG(sigma && act && g_mu && g_sigma, "tsrl_sac_sample_bwd: null pointer");
    TSRL_CHECK_ARG(g_act || g_logp, "tsrl_sac_sample_bwd: g_act and g_logp are both null");
    const int64_t n = b * A;
    hipLaunchKernelGGL(sac_sample_bwd_kernel, dim3(blocks_of(n, TPB)), dim3(TPB), 0,
                       as_stream(stream), sigma, eps, act, g_act, g_logp, n, A, g_mu, g_sigma);
    TSRL_LAUNCH_CHECK("tsrl_sac_sample_bwd");
    return 0;
}

extern "C" int tsrl_sac_target(const float* q1, const float* q2, const float* log_prob,
                               const float* alpha, int64_t b, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_sac_target: need b >= 1");
    TSRL_CHECK_ARG(q1 && q2 && log_prob && alpha && out, "tsrl_sac_target: null pointer");
    hipLaunchKernelGGL(sac_target_kernel, dim3(blocks_of(b, TPB)), dim3(TPB), 0,
                       as_stream(stream), q1, q2, log_prob, alpha, b, out);
    TSRL_LAUNCH_CHECK("tsrl_sac_target");
    return 0;
}

extern "C" int tsrl_sac_actor_loss_fwd_bwd(const float* q1, const float* q2,
                                           const float* log_prob, const float* alpha,
                                           const float* log_alpha, double target_entropy,
                                           int64_t b, float* g_q1, float* g_q2, float* g_logp,
                                           double* partials, float* loss, float* g_log_alpha,
                                           void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB,
                   "tsrl_sac_actor_loss_fwd_bwd: need b >= 1");
    TSRL_CHECK_ARG(q1 && q2 && log_prob && alpha && g_q1 && g_q2 && g_logp && loss,
                   "tsrl_sac_actor_loss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(!log_alpha || g_log_alpha,
                   "tsrl_sac_actor_loss_fwd_bwd: log_alpha needs g_log_alpha");
    const hipStream_t st = as_stream(stream);
    const ActorAlphaLosses fin{(double)b, 1.0, log_alpha, loss, g_log_alpha};
    return launch_loss<2>("tsrl_sac_actor_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(sac_actor_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q1, q2, log_prob,
                           alpha, (float)target_entropy, b, 1.0f / (float)b, g_q1, g_q2, g_logp,
                           partials, fin);
    });
}
