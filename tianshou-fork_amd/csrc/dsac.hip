// DiscreteSACPolicy (tianshou/policy/modelfree/discrete_sac.py): the glue around the actor and
// critic forwards.  In torch Categorical(logits=...) with its .probs and .entropy(), the min
// over the critics and the weighted sums are about a dozen launches over a few hundred rows of
// <= 18 actions, taken in _target_q and again, with their autograd backward, in learn(): launch
// latency, as in ddpg.hip and sac.hip.
//   dsac_target_kernel       _target_q after the three forwards (discrete_sac.py:93-97)
//   dsac_q_loss_kernel       both critics' TD error, loss and [b, A] gradient (:108-124)
//   dsac_actor_loss_kernel   the actor loss, the temperature loss and every gradient of both
//                            (:127-144), summed in loss_sum.h's order
// Per row, in f64 on the f32 inputs: m = max_j l_j, S = sum_j exp(l_j - m), lp_j = l_j - m -
// log S, p_j = exp(lp_j), H = -sum_j p_j lp_j (a term with p_j == 0 is exactly 0), qm_j =
// min(q1_j, q2_j) (a NaN handed through), V = sum_j p_j qm_j: what Categorical(logits=l)
// normalises to.  A -inf logit (an illegal action masked out by the actor) follows torch: p_j = 0,
// nothing added to H or V (0 * a finite q), and in the actor loss a gradient of exactly 0, through
// the clamp of lp_j at f32's lowest value that torch's entropy() applies.  A row of all -inf, a
// +inf or a NaN logit make that row's outputs and the losses NaN, as in torch, and no other row's.
//
// Row mapping: a group of G lanes shares one row, G = the power of two >= A capped at one wave
// (A = 1: 1, A = 18: 32, A > 64: 64 with a loop), lane g of the group on columns g, g + G, ...
// Groups are aligned inside a wave, so the group reductions are xor butterflies below G; a wave
// reads 64 / G consecutive rows, i.e. one contiguous span of the row-major table.  The
// temperature is read from device memory: it changes inside a replayed graph.
#include "loss_sum.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;
constexpr double kF32Min = -3.4028234663852886e+38;  // torch.finfo(torch.float32).min

// Butterflies over the G lanes of a group: every lane ends with the same bits (each level adds
// or compares the same two values on both sides).
__device__ __forceinline__ double group_sum(double v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
    for (int off = G >> 1; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, kWave);
        v = (o > v || o != o) ? o : v;  // a NaN logit poisons the row, as torch's logsumexp
    }
    return v;
}

struct RowStats {
    double shift;  // m + log S: lp_j = l_j - shift
    double H, V;
};

// Every lane of the group calls this (an invalid row with valid = false: nothing is read).
__device__ __forceinline__ RowStats row_stats(const float* __restrict__ l,
                                              const float* __restrict__ q1,
                                              const float* __restrict__ q2, int64_t A, int g,
                                              int G, bool valid) {
#pragma clang fp contract(off)
    float mx = -INFINITY;
    if (valid)
        for (int64_t j = g; j < A; j += G) {
            const float v = l[j];
            mx = (v > mx || v != v) ? v : mx;
        }
    const double m = (double)group_max(mx, G);
    double s = 0.0;
    if (valid)
        for (int64_t j = g; j < A; j += G) s += exp((double)l[j] - m);
    s = group_sum(s, G);
    RowStats st;
    st.shift = m + log(s);
    double h = 0.0, v = 0.0;
    if (valid)
        for (int64_t j = g; j < A; j += G) {
            const double lp = (double)l[j] - st.shift;
            const double p = exp(lp);
            h -= p == 0.0 ? 0.0 : p * lp;
            v += p * (double)min_nan(q1[j], q2[j]);
        }
    st.H = group_sum(h, G);
    st.V = group_sum(v, G);
    return st;
}

// TPB / G rows per workgroup.
__global__ __launch_bounds__(TPB) void dsac_target_kernel(
    const float* __restrict__ logits, const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ alpha, int64_t b, int64_t A, int G, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    const int g = t & (G - 1);
    const int64_t r = (int64_t)blockIdx.x * (TPB / G) + t / G;
    const bool valid = r < b;
    const int64_t o = valid ? r * A : 0;
    const RowStats st = row_stats(logits + o, q1 + o, q2 + o, A, g, G, valid);
    if (valid && g == 0) {
        const double ah = (double)alpha[0] * st.H;
        out[r] = (float)(st.V + ah);
    }
}

// One workgroup = 256 rows, one row per lane: its TD errors, loss terms and the one non-zero
// gradient entry per critic (the taken action's Q is one gathered element per row); the
// [rows, A] gradient tiles are then written by the whole workgroup in storage order (zeros off
// the taken action), as dqn.hip's td_fwd_bwd_kernel.  s[k] = sum(td_k^2 * weight), in
// loss_sum.h's order.
__global__ __launch_bounds__(TPB) void dsac_q_loss_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ weight, int64_t b, int64_t A,
    float inv_b, float* __restrict__ grad1, float* __restrict__ grad2,
    float* __restrict__ td_out, double* __restrict__ partials, MeanLosses<2> fin) {
#pragma clang fp contract(off)
    __shared__ float s_g[2][TPB];
    __shared__ int s_a[TPB];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * TPB;
    const int nrows = (int)min((int64_t)TPB, b - r0);
    double term[2] = {0.0, 0.0};
    float gk[2] = {0.0f, 0.0f};
    int a = -1;
    if (t < nrows) {
        const int64_t r = r0 + t;
        const int64_t a64 = act[r];
        a = (a64 >= 0 && a64 < A) ? (int)a64 : -1;  // invalid action -> NaN loss, no gradient
        const float ret = returns[r];
        const float w = weight ? weight[r] : 1.0f;
        const float td1 = (a >= 0 ? q1[r * A + a] : NAN) - ret;
        const float td2 = (a >= 0 ? q2[r * A + a] : NAN) - ret;
        term[0] = (double)(td1 * td1 * w);
        term[1] = (double)(td2 * td2 * w);
        gk[0] = 2.0f * td1 * w * inv_b;
        gk[1] = 2.0f * td2 * w * inv_b;
        td_out[r] = (td1 + td2) / 2.0f;
    }
    s_g[0][t] = gk[0];
    s_g[1][t] = gk[1];
    s_a[t] = a;
    double s[2];
    block_sums<2>(term, s);  // its barrier also publishes s_g and s_a
    const int64_t nel = (int64_t)nrows * A;
    float* g1 = grad1 + r0 * A;
    float* g2 = grad2 + r0 * A;
    for (int64_t f = t; f < nel; f += TPB) {
        const int row = (int)(f / A);
        const bool hit = (int)(f - (int64_t)row * A) == s_a[row];
        g1[f] = hit ? s_g[0][row] : 0.0f;
        g2[f] = hit ? s_g[1][row] : 0.0f;
    }
    losses_or_partials<2>(s, partials, fin);
}

// One workgroup = 256 rows in G passes of TPB / G rows each; the first lane of a group carries
// its rows' loss terms: s[0] = sum(alpha H + V), s[1] = sum(target_entropy - H), a lane's
// passes in pass order and then loss_sum.h's order.
__global__ __launch_bounds__(TPB) void dsac_actor_loss_kernel(
    const float* __restrict__ logits, const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ alpha, double target_entropy, int64_t b, int64_t A, int G,
    double inv_b, float* __restrict__ g_logits, double* __restrict__ partials,
    ActorAlphaLosses fin) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    const int g = t & (G - 1);
    const int rpp = TPB / G;  // rows per pass
    const double al = (double)alpha[0];
    double term[2] = {0.0, 0.0};
    for (int pass = 0; pass < G; ++pass) {
        const int64_t first = (int64_t)blockIdx.x * TPB + pass * rpp;
        if (first >= b) break;  // uniform over the workgroup
        const int64_t r = first + t / G;
        const bool valid = r < b;  // uniform over a group
        const int64_t o = valid ? r * A : 0;
        const float* l = logits + o;
        const RowStats st = row_stats(l, q1 + o, q2 + o, A, g, G, valid);
        if (valid) {
            if (g == 0) {
                const double ah = al * st.H;
                term[0] += ah + st.V;
                term[1] += target_entropy - st.H;
            }
            for (int64_t j = g; j < A; j += G) {
                const double lp = (double)l[j] - st.shift;
                const double p = exp(lp);
                const double adv = (double)min_nan(q1[o + j], q2[o + j]) - st.V;
                // torch's entropy() clamps the normalised logit at f32's lowest value: a -inf
                // (masked) entry has p = 0 and a finite ent, so its gradient is 0 * finite = 0
                // and not 0 * inf.  Every lp above that value is left as it is, and below it p
                // is 0 already; a NaN lp has a NaN p.
                const double ent = al * (fmax(lp, kF32Min) + st.H);
                g_logits[o + j] = (float)(-inv_b * (p * (adv - ent)));
            }
        }
    }
    double s[2];
    block_sums<2>(term, s);
    losses_or_partials<2>(s, partials, fin);
}

// The power of two >= A, at most one wave.
inline int group_lanes(int64_t A) {
    int G = 1;
    while (G < kWave && G < A) G <<= 1;
    return G;
}

constexpr int64_t kMaxRows = (int64_t)1 << 31;     // 2^31 workgroups of >= 4 rows stay in range
constexpr int64_t kMaxActions = (int64_t)1 << 24;

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_dsac_target(const float* logits, const float* q1, const float* q2,
                                const float* alpha, int64_t b, int64_t A, float* out,
                                void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < kMaxRows && A >= 1 && A < kMaxActions,
                   "tsrl_dsac_target: need b >= 0 and num_actions >= 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(logits && q1 && q2 && alpha && out, "tsrl_dsac_target: null pointer");
    const int G = group_lanes(A);
    const int64_t rpb = TPB / G;
    hipLaunchKernelGGL(dsac_target_kernel, dim3((unsigned)((b + rpb - 1) / rpb)), dim3(TPB), 0,
                       as_stream(stream), logits, q1, q2, alpha, b, A, G, out);
    TSRL_LAUNCH_CHECK("tsrl_dsac_target");
    return 0;
}

extern "C" int tsrl_dsac_q_loss_fwd_bwd(const float* q1, const float* q2, const int64_t* act,
                                        const float* returns, const float* weight, int64_t b,
                                        int64_t A, float* grad1, float* grad2, float* td_out,
                                        double* partials, float* loss, float* total,
                                        void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < kMaxRows && A >= 1 && A < kMaxActions,
                   "tsrl_dsac_q_loss_fwd_bwd: need b >= 0 and num_actions >= 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(q1 && q2 && act && returns && grad1 && grad2 && td_out && loss,
                   "tsrl_dsac_q_loss_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const MeanLosses<2> fin{(double)b, 1.0f, loss, total};
    return launch_loss<2>("tsrl_dsac_q_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(dsac_q_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q1, q2, act, returns,
                           weight, b, A, 1.0f / (float)b, grad1, grad2, td_out, partials, fin);
    });
}

extern "C" int tsrl_dsac_actor_loss_fwd_bwd(const float* logits, const float* q1,
                                            const float* q2, const float* alpha,
                                            const float* log_alpha, double target_entropy,
                                            int64_t b, int64_t A, float* g_logits,
                                            double* partials, float* loss, float* g_log_alpha,
                                            void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < kMaxRows && A >= 1 && A < kMaxActions,
                   "tsrl_dsac_actor_loss_fwd_bwd: need b >= 0 and num_actions >= 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(logits && q1 && q2 && alpha && g_logits && loss,
                   "tsrl_dsac_actor_loss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(!log_alpha || g_log_alpha,
                   "tsrl_dsac_actor_loss_fwd_bwd: log_alpha needs g_log_alpha");
    const hipStream_t st = as_stream(stream);
    const ActorAlphaLosses fin{(double)b, -1.0, log_alpha, loss, g_log_alpha};
    return launch_loss<2>("tsrl_dsac_actor_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(dsac_actor_loss_kernel, dim3(nblk), dim3(TPB), 0, st, logits, q1, q2,
                           alpha, target_entropy, b, A, group_lanes(A), 1.0 / (double)b, g_logits,
                           partials, fin);
    });
}
