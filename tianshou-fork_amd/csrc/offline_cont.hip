// The continuous offline policies (tianshou/policy/imitation/cql.py, td3_bc.py): the glue around
// the actor and critic forwards.  With batch size b and R repeated actions per row the reference's
// CQL update repeats observations into b R rows, draws random actions, evaluates each critic
// four times and closes with a three-way logsumexp, a Lagrange multiplier and two clipped steps:
// about thirty torch launches over a few thousand elements, launch latency as in ddpg.hip.
//   cql_expand_kernel        every repeated row the update needs and the random actions, one
//                            launch: a row gather, a wave owns whole output rows
//   cql_target_kernel        rew + gamma (1 - done) (min(Q1, Q2) - alpha log_prob)  (cql.py:185-194)
//   cql_loss_kernel          both critics' MSE and CQL terms, the multiplier's loss and every
//                            gradient (cql.py:198-260), six f64 sums in loss_sum.h's order
//   td3bc_actor_loss_kernel  -lmbda mean(q) + mse(act, data_act), lmbda = alpha / mean|q| held
//   td3bc_fold_kernel        constant (td3_bc.py:91-96); g_q needs the batch sums first
// The temperature and the multiplier are read from device memory: both move inside a replayed
// graph.  No float atomics: every sum is block_sums' fixed order.
#include "loss_sum.h"

#include <math.h>

#include <type_traits>

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;

// One sub-group of 2^lpr_log2 lanes = one job n = i R + j (source row i, repeat j): the source
// rows obs[i] and obs_next[i] are read once and stored to the five places the update reads
// them from, then the job's random action row is scaled.  VEC: D % 4 == 0 and every base is
// 16-byte aligned, so every row start is; the rows move as float4.  Else float by float.
template <bool VEC>
__global__ __launch_bounds__(TPB) void cql_expand_kernel(
    const float* __restrict__ obs, const float* __restrict__ obs_next,
    const float* __restrict__ u, float lo, float span, int64_t nR, int64_t R, int64_t D,
    int64_t A, int lpr_log2, float* __restrict__ actor_in, float* __restrict__ critic_obs,
    float* __restrict__ critic_act) {
#pragma clang fp contract(off)
    using T = typename std::conditional<VEC, float4, float>::type;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (TPB / kWave) + threadIdx.x / kWave;
    const int64_t n = wave * (kWave >> lpr_log2) + (lane >> lpr_log2);
    if (n >= nR) return;
    const int lpr = 1 << lpr_log2;
    const int c0 = lane & (lpr - 1);
    const int64_t src = n / R;
    const int64_t nv = VEC ? D / 4 : D;
    const T* s = reinterpret_cast<const T*>(obs + src * D);
    const T* sn = reinterpret_cast<const T*>(obs_next + src * D);
    T* a0 = reinterpret_cast<T*>(actor_in + n * D);
    T* a1 = reinterpret_cast<T*>(actor_in + (nR + n) * D);
    T* q0 = reinterpret_cast<T*>(critic_obs + n * D);
    T* q1 = reinterpret_cast<T*>(critic_obs + (nR + n) * D);
    T* q2 = reinterpret_cast<T*>(critic_obs + (2 * nR + n) * D);
    for (int64_t c = c0; c < nv; c += lpr) {
        const T v = s[c];
        const T w = sn[c];
        a0[c] = v;
        a1[c] = w;
        q0[c] = v;
        q1[c] = v;
        q2[c] = v;
    }
    for (int64_t j = c0; j < A; j += lpr) {
        const float p = u[n * A + j] * span;
        critic_act[n * A + j] = lo + p;
    }
}

__global__ __launch_bounds__(TPB) void cql_target_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ log_prob,
    const float* __restrict__ alpha, const float* __restrict__ rew, const float* __restrict__ done,
    float gamma, int64_t b, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    const float p = alpha[0] * log_prob[r];
    const float t = min_nan(q1[r], q2[r]) - p;
    const float c = gamma * (1.0f - done[r]);
    const float ct = c * t;
    out[r] = rew[r] + ct;
}

// clamp(exp(cql_log_alpha), alpha_min, alpha_max) in f32, as torch evaluates it; `inside`: the
// clamp hands the gradient through (torch: min <= x <= max).
__device__ __forceinline__ float cql_alpha_of(const float* log_alpha, float amin, float amax,
                                              float* e_out, bool* inside) {
    const float e = expf(log_alpha[0]);
    *e_out = e;
    *inside = e >= amin && e <= amax;
    return e < amin ? amin : (e > amax ? amax : e);
}

// s[0..2) = sum_n lse_i, s[2..4) = sum_r (q_i - target)^2, s[4..6) = sum_r q_i.
struct CqlLosses {
    double n, b, w, T, thr;
    float amin, amax;
    const float* log_alpha;  // null: no Lagrange multiplier
    float* loss;             // [2]: critic1, critic2
    float* lagrange;         // [2]: cql_alpha_loss, cql_alpha
    float* g_log_alpha;      // [1]
    __device__ void operator()(const double* s) const {
        double a = 1.0, e = 0.0;
        bool inside = false;
        if (log_alpha) {
            float ef;
            a = (double)cql_alpha_of(log_alpha, amin, amax, &ef, &inside);
            e = (double)ef;
        }
        double raw[2], cql[2];
        for (int i = 0; i < 2; ++i) {
            raw[i] = s[i] / n * w * T - s[4 + i] / b * w;
            cql[i] = log_alpha ? a * (raw[i] - thr) : raw[i];
            loss[i] = (float)(s[2 + i] / b + cql[i]);
        }
        if (log_alpha) {
            lagrange[0] = (float)(-0.5 * (cql[0] + cql[1]));
            lagrange[1] = (float)a;
            g_log_alpha[0] =
                inside ? (float)(-0.5 * ((raw[0] - thr) + (raw[1] - thr)) * e) : 0.0f;
        }
    }
};

// Max-subtracted logsumexp of three values with its softmax weights, f64.  An infinite maximum
// is not subtracted (torch.logsumexp's rule), so three -inf give -inf and not NaN.
__device__ __forceinline__ double lse3(const double x[3], double p[3]) {
    double m = x[0];
    if (x[1] > m) m = x[1];
    if (x[2] > m) m = x[2];
    const double ms = (m == INFINITY || m == -INFINITY) ? 0.0 : m;
    double sum = 0.0;
    for (int k = 0; k < 3; ++k) {
        p[k] = exp(x[k] - ms);
        sum += p[k];
    }
    for (int k = 0; k < 3; ++k) p[k] = p[k] / sum;
    return ms + log(sum);
}

// One lane = one of the n = b R repeated rows, both critics; the first b lanes also carry their
// data row's MSE and q terms.  No gradient depends on a batch mean, so all are written here.
__global__ __launch_bounds__(TPB) void cql_loss_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ target,
    const float* __restrict__ v1, const float* __restrict__ v2, const float* __restrict__ log_pi,
    const float* __restrict__ log_alpha, double rand_logp, double T, double w, float amin,
    float amax, int64_t b, int64_t n, float* __restrict__ g_q1, float* __restrict__ g_q2,
    float* __restrict__ g_v1, float* __restrict__ g_v2, double* __restrict__ partials,
    CqlLosses fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double a = 1.0;
    if (log_alpha) {
        float e;
        bool inside;
        a = (double)cql_alpha_of(log_alpha, amin, amax, &e, &inside);
    }
    const double aw = a * w;
    double term[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (r < n) {
        const double sub[3] = {rand_logp, (double)log_pi[r], (double)log_pi[n + r]};
        const float* vs[2] = {v1, v2};
        float* gs[2] = {g_v1, g_v2};
        const double gscale = aw / (double)n;
        for (int i = 0; i < 2; ++i) {
            double x[3], p[3];
            for (int k = 0; k < 3; ++k) x[k] = ((double)vs[i][k * n + r] - sub[k]) / T;
            term[i] = lse3(x, p);
            for (int k = 0; k < 3; ++k) gs[i][k * n + r] = (float)(gscale * p[k]);
        }
    }
    if (r < b) {
        const double t = (double)target[r];
        const double bd = (double)b;
        const double d1 = (double)q1[r] - t, d2 = (double)q2[r] - t;
        term[2] = d1 * d1;
        term[3] = d2 * d2;
        term[4] = (double)q1[r];
        term[5] = (double)q2[r];
        g_q1[r] = (float)(2.0 * d1 / bd - aw / bd);
        g_q2[r] = (float)(2.0 * d2 / bd - aw / bd);
    }
    double s[6];
    block_sums<6>(term, s);
    losses_or_partials<6>(s, partials, fin);
}

// s[0] = sum q, s[1] = sum |q|, s[2] = sum (act - data_act)^2 over all b A elements.
struct Td3bcSums {
    double b, bA, alpha;
    // loss and lmbda / b of the finished sums
    __device__ double finish(const double* s, float* loss) const {
        const double lmbda = alpha / (s[1] / b);
        if (loss) loss[0] = (float)(-lmbda * (s[0] / b) + s[2] / bA);
        return lmbda / b;
    }
};

// One lane = one row.  g_act is written with the terms; g_q = -lmbda / b is uniform and needs
// the sums: one workgroup publishes it through LDS after block_sums, more leave partials.
__global__ __launch_bounds__(TPB) void td3bc_actor_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ act, const float* __restrict__ data_act,
    int64_t b, int64_t A, float* __restrict__ g_q, float* __restrict__ g_act,
    double* __restrict__ partials, float* __restrict__ loss, Td3bcSums fin) {
    __shared__ double coef;
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[3] = {0.0, 0.0, 0.0};
    if (r < b) {
        const double x = (double)q[r];
        term[0] = x;
        term[1] = fabs(x);
        const double gs = 2.0 / fin.bA;
        for (int64_t j = 0; j < A; ++j) {
            const double d = (double)act[r * A + j] - (double)data_act[r * A + j];
            term[2] += d * d;
            g_act[r * A + j] = (float)(gs * d);
        }
    }
    double s[3];
    block_sums<3>(term, s);
    if (gridDim.x > 1) {
        if (threadIdx.x == 0)
            for (int k = 0; k < 3; ++k) partials[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
        return;
    }
    if (threadIdx.x == 0) coef = fin.finish(s, loss);
    __syncthreads();
    if (r < b) g_q[r] = (float)(-coef);
}

// Beyond one workgroup: every lane sums the partials in block order (loss_fold_kernel's order,
// so all lanes hold the same bits) and writes its row of g_q; lane 0 of block 0 the loss.
__global__ __launch_bounds__(TPB) void td3bc_fold_kernel(
    const double* __restrict__ partials, int64_t nblk, int64_t b, float* __restrict__ g_q,
    float* __restrict__ loss, Td3bcSums fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double s[3];
    for (int k = 0; k < 3; ++k) {
        s[k] = 0.0;
        for (int64_t i = 0; i < nblk; ++i) s[k] += partials[(int64_t)k * nblk + i];
    }
    const double coef = fin.finish(s, r == 0 ? loss : nullptr);
    if (r < b) g_q[r] = (float)(-coef);
}

inline unsigned blocks_of(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_cql_expand(const float* obs, const float* obs_next, const float* u, double lo,
                               double hi, int64_t b, int64_t R, int64_t D, int64_t A,
                               float* actor_in, float* critic_obs, float* critic_act,
                               void* stream) {
    TSRL_CHECK_ARG(b >= 1 && R >= 1 && D >= 1 && A >= 1, "tsrl_cql_expand: need b, R, D, A >= 1");
    TSRL_CHECK_ARG(b < ((int64_t)1 << 31) / R && D < ((int64_t)1 << 31) && A < ((int64_t)1 << 31),
                   "tsrl_cql_expand: b R, D and A must stay below 2^31");
    TSRL_CHECK_ARG(obs && obs_next && u && actor_in && critic_obs && critic_act,
                   "tsrl_cql_expand: null pointer");
    const int64_t nR = b * R;
    const bool vec = D % 4 == 0 && aligned16(obs) && aligned16(obs_next) && aligned16(actor_in) &&
                     aligned16(critic_obs);
    const int64_t nv = vec ? D / 4 : D;
    int lpr_log2 = 0;  // lanes per row: the least power of two covering the row, a wave at most
    while (lpr_log2 < 6 && ((int64_t)1 << lpr_log2) < nv) ++lpr_log2;
    const int64_t rows_per_block = (int64_t)(TPB / kWave) * (kWave >> lpr_log2);
    const dim3 grid(blocks_of(nR, rows_per_block));
    const float flo = (float)lo, span = (float)(hi - lo);
    if (vec)
        hipLaunchKernelGGL(cql_expand_kernel<true>, grid, dim3(TPB), 0, as_stream(stream), obs,
                           obs_next, u, flo, span, nR, R, D, A, lpr_log2, actor_in, critic_obs,
                           critic_act);
    else
        hipLaunchKernelGGL(cql_expand_kernel<false>, grid, dim3(TPB), 0, as_stream(stream), obs,
                           obs_next, u, flo, span, nR, R, D, A, lpr_log2, actor_in, critic_obs,
                           critic_act);
    TSRL_LAUNCH_CHECK("tsrl_cql_expand");
    return 0;
}

extern "C" int tsrl_cql_target(const float* q1, const float* q2, const float* log_prob,
                               const float* alpha, const float* rew, const float* done,
                               double gamma, int64_t b, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_cql_target: need b >= 1");
    TSRL_CHECK_ARG(q1 && q2 && log_prob && alpha && rew && done && out,
                   "tsrl_cql_target: null pointer");
    hipLaunchKernelGGL(cql_target_kernel, dim3(blocks_of(b, TPB)), dim3(TPB), 0,
                       as_stream(stream), q1, q2, log_prob, alpha, rew, done, (float)gamma, b, out);
    TSRL_LAUNCH_CHECK("tsrl_cql_target");
    return 0;
}

extern "C" int tsrl_cql_loss_fwd_bwd(const float* q1, const float* q2, const float* target,
                                     const float* v1, const float* v2, const float* log_pi,
                                     const float* cql_log_alpha, double temperature,
                                     double cql_weight, double lagrange_threshold,
                                     double alpha_min, double alpha_max, int64_t act_dim,
                                     int with_lagrange, int64_t b, int64_t R, float* g_q1,
                                     float* g_q2, float* g_v1, float* g_v2, double* partials,
                                     float* loss, float* lagrange, float* g_cql_log_alpha,
                                     void* stream) {
    TSRL_CHECK_ARG(b >= 1 && R >= 1 && act_dim >= 1 && b < ((int64_t)1 << 31) / R,
                   "tsrl_cql_loss_fwd_bwd: need b, R, act_dim >= 1 and b R < 2^31");
    TSRL_CHECK_ARG(q1 && q2 && target && v1 && v2 && log_pi && g_q1 && g_q2 && g_v1 && g_v2 && loss,
                   "tsrl_cql_loss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(!with_lagrange || (cql_log_alpha && lagrange && g_cql_log_alpha),
                   "tsrl_cql_loss_fwd_bwd: with_lagrange needs cql_log_alpha, lagrange and "
                   "g_cql_log_alpha");
    TSRL_CHECK_ARG(temperature != 0.0, "tsrl_cql_loss_fwd_bwd: temperature is zero");
    const int64_t n = b * R;
    const float* la = with_lagrange ? cql_log_alpha : nullptr;
    const float amin = (float)alpha_min, amax = (float)alpha_max;
    const double rand_logp = log(pow(0.5, (double)act_dim));  // np.log(0.5 ** act_dim)
    const hipStream_t st = as_stream(stream);
    const CqlLosses fin{(double)n, (double)b, cql_weight, temperature, lagrange_threshold,
                        amin,      amax,      la,         loss,        lagrange,
                        g_cql_log_alpha};
    return launch_loss<6>("tsrl_cql_loss_fwd_bwd", n, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(cql_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q1, q2, target, v1, v2,
                           log_pi, la, rand_logp, temperature, cql_weight, amin, amax, b, n, g_q1,
                           g_q2, g_v1, g_v2, partials, fin);
    });
}

extern "C" int tsrl_td3bc_actor_loss_fwd_bwd(const float* q, const float* act,
                                             const float* data_act, double alpha, int64_t b,
                                             int64_t A, float* g_q, float* g_act,
                                             double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && A >= 1 && A < ((int64_t)1 << 31) && b < ((int64_t)1 << 31) / A,
                   "tsrl_td3bc_actor_loss_fwd_bwd: need b, A >= 1 and b A < 2^31");
    TSRL_CHECK_ARG(q && act && data_act && g_q && g_act && loss,
                   "tsrl_td3bc_actor_loss_fwd_bwd: null pointer");
    const int64_t nblk = loss_blocks(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "tsrl_td3bc_actor_loss_fwd_bwd: b > %d needs partials",
                   TPB);
    const hipStream_t st = as_stream(stream);
    const Td3bcSums fin{(double)b, (double)b * (double)A, alpha};
    hipLaunchKernelGGL(td3bc_actor_loss_kernel, dim3((unsigned)nblk), dim3(TPB), 0, st, q, act,
                       data_act, b, A, g_q, g_act, partials, loss, fin);
    TSRL_LAUNCH_CHECK("tsrl_td3bc_actor_loss_fwd_bwd");
    if (nblk > 1) {
        hipLaunchKernelGGL(td3bc_fold_kernel, dim3((unsigned)nblk), dim3(TPB), 0, st, partials,
                           nblk, b, g_q, loss, fin);
        TSRL_LAUNCH_CHECK("tsrl_td3bc_actor_loss_fwd_bwd (fold)");
    }
    return 0;
}
