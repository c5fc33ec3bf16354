// The discrete offline policies' passes around their forwards: DiscreteBCQPolicy
// (tianshou/policy/imitation/discrete_bcq.py), DiscreteCQLPolicy (discrete_cql.py) and
// DiscreteCRRPolicy (discrete_crr.py).
//   bcq_select:  forward()'s thresholded action (discrete_bcq.py:97-99) and _target_q's gather
//                (:78-80) in one launch;
//   bcq_loss:    learn()'s three terms with both gradients (:110-118);
//   cql_qr_loss: QR-DQN's pairwise Huber loss plus the CQL regulariser over the quantile means
//                (discrete_cql.py:57-76), with a dense [b, A, N] gradient;
//   crr_loss:    the critic, actor and CQL terms of discrete_crr.py:88-117 with both gradients,
//                the gradient through the undetached coefficient included.  The reference's
//                actor loss is a product of two batch means (see CrrLosses), so the gradients
//                are a second pass after the sums.
// bcq_* and crr_loss are one row per lane, 256 rows per workgroup (loss_sum.h's split): b is at
// most a few hundred and A at most a few dozen, so the cost is launch latency and a lane walks
// its own row of A floats (uncoalesced).  cql_qr_loss is one workgroup per row, as qr_loss_kernel
// of dqn_dist.hip.  All per-row arithmetic is f64, rounded once; sums run in a fixed order, no
// atomics: bit-identical between runs.
#include <float.h>

#include "loss_sum.h"
#include "qr_pair.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;
constexpr int NW = TPB / kWave;
constexpr int64_t kMaxN = TSRL_DIST_MAX_N;
constexpr int64_t kMaxA = TSRL_CQL_MAX_ACTIONS;

// torch's max / argmax over a row: the first index of the maximum, the first NaN wins.
__device__ __forceinline__ bool beats(float v, float best) {
    return v > best || (v != v && best == best);
}

// The shift of a max-subtracted logsumexp: the maximum, or 0 when that is not finite (torch's
// rule: a row of -inf gives -inf, a NaN travels through the exponentials).
__device__ __forceinline__ double lse_shift(double m) { return fabs(m) <= DBL_MAX ? m : 0.0; }

// max over x[0..A) that ignores NaN (they reach the sum of exponentials instead).
__device__ __forceinline__ double row_max(const float* __restrict__ x, int64_t A) {
    double m = -INFINITY;
    for (int64_t a = 0; a < A; ++a) m = fmax(m, (double)x[a]);
    return lse_shift(m);
}

// logsumexp(x[0..A)) around the shift m.
__device__ __forceinline__ double row_lse(const float* __restrict__ x, int64_t A, double m) {
    double s = 0.0;
    for (int64_t a = 0; a < A; ++a) s += exp((double)x[a] - m);
    return m + log(s);
}

__global__ __launch_bounds__(TPB) void bcq_select_kernel(
    const float* __restrict__ q, const float* __restrict__ logits, float log_tau,
    const float* __restrict__ q_eval, int paper, int64_t b, int64_t A,
    int64_t* __restrict__ act, float* __restrict__ val) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    const float* l = logits + r * A;
    const float* qr = q + r * A;
    float mx = l[0];
    for (int64_t a = 1; a < A; ++a)
        if (beats(l[a], mx)) mx = l[a];
    int64_t arg = -1;
    float best = 0.0f;
    for (int64_t a = 0; a < A; ++a) {
        const float ratio = l[a] - mx;  // torch's f32 subtraction and f32 comparison
        if (ratio < log_tau) continue;  // a NaN ratio compares false: allowed
        if (arg < 0) {
            arg = a;
            if (!paper) break;  // reference: the first allowed action
            best = qr[a];
        } else if (beats(qr[a], best)) {
            best = qr[a];
            arg = a;
        }
    }
    if (arg < 0) arg = 0;  // unreachable: the maximum has ratio 0, a NaN maximum allows all
    act[r] = arg;
    if (val) val[r] = q_eval[r * A + arg];
}

// loss[0..4) = total, q, i, reg of s = (sum smooth-L1, sum nll, sum logits^2).
struct BcqLosses {
    double b, n_logits, weight_reg;
    float* loss;
    __device__ void operator()(const double* s) const {
        const double ql = s[0] / b, il = s[1] / b, rl = s[2] / n_logits;
        loss[0] = (float)(ql + il + weight_reg * rl);
        loss[1] = (float)ql;
        loss[2] = (float)il;
        loss[3] = (float)rl;
    }
};

__global__ __launch_bounds__(TPB) void bcq_loss_kernel(
    const float* __restrict__ q, const float* __restrict__ logits,
    const int64_t* __restrict__ act, const float* __restrict__ returns, int64_t b, int64_t A,
    double weight_reg, float* __restrict__ grad_q, float* __restrict__ grad_l,
    double* __restrict__ partials, BcqLosses fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[3] = {0.0, 0.0, 0.0};
    if (r < b) {
        const float* l = logits + r * A;
        float* gq = grad_q + r * A;
        float* gl = grad_l + r * A;
        const int64_t a64 = act[r];
        const int64_t at = (a64 >= 0 && a64 < A) ? a64 : -1;  // invalid: NaN losses, no q grad
        const double inv_b = 1.0 / (double)b;
        const double reg_scale = 2.0 * weight_reg / ((double)b * (double)A);
        const double m = row_max(l, A);
        const double lse = row_lse(l, A, m);
        double sq = 0.0;
        for (int64_t a = 0; a < A; ++a) {
            const double la = (double)l[a];
            sq += la * la;
            const double p = exp(la - lse);
            gl[a] = (float)((p - (a == at ? 1.0 : 0.0)) * inv_b + reg_scale * la);
            gq[a] = 0.0f;
        }
        term[2] = sq;
        if (at >= 0) {
            const double x = (double)q[r * A + at] - (double)returns[r];
            const double ax = fabs(x);
            term[0] = ax < 1.0 ? 0.5 * x * x : ax - 0.5;
            // torch's smooth_l1 backward: x in (-1, 1) -> x, else sign(x); a NaN stays NaN
            gq[at] = (float)((x != x ? x : fmin(fmax(x, -1.0), 1.0)) * inv_b);
            term[1] = lse - (double)l[at];
        } else {
            term[0] = term[1] = (double)NAN;
        }
    }
    double s[3];
    block_sums<3>(term, s);
    losses_or_partials<3>(s, partials, fin);
}

enum { kCrrExp = 0, kCrrBinary = 1, kCrrAll = 2 };

// s = the row sums of (nlp, coef, critic, cql).  The reference multiplies log_prob [b] by the
// coefficient [b, 1], which broadcasts to [b, b]: its actor loss is mean(nlp) * mean(coef).
// loss[0..4) = total, actor, critic, cql; means[0..2) = mean(nlp), mean(coef) for the gradient
// pass.
struct CrrLosses {
    double b, min_q_weight;
    float* loss;
    double* means;
    __device__ void operator()(const double* s) const {
        const double nm = s[0] / b, cm = s[1] / b, cl = s[2] / b, ql = s[3] / b;
        const double al = nm * cm;
        means[0] = nm;
        means[1] = cm;
        loss[0] = (float)(al + cl + min_q_weight * ql);
        loss[1] = (float)al;
        loss[2] = (float)cl;
        loss[3] = (float)ql;
    }
};

// What both CRR passes need of one row (discrete_crr.py:88-117).
struct CrrRow {
    int64_t at;                                // the taken action, -1 when outside [0, A)
    double lse_l, lse_q, V, qa, nlp, c, dc, dq;  // dc = d coef / d adv, dq = q_t - target
};

__device__ __forceinline__ CrrRow crr_row(const float* __restrict__ qr, const float* __restrict__ l,
                                          int64_t a64, const float* __restrict__ tl,
                                          const float* __restrict__ tq, float rew, uint8_t done,
                                          int64_t A, double gamma, int mode, double beta,
                                          double ub) {
    CrrRow o;
    o.at = (a64 >= 0 && a64 < A) ? a64 : -1;
    double ev = 0.0;  // the target policy's expected target Q, 0 on a done row
    if (!done) {
        const double tm = row_max(tl, A);
        double se = 0.0, sv = 0.0;
        for (int64_t a = 0; a < A; ++a) {
            const double e = exp((double)tl[a] - tm);
            se += e;
            sv += e * (double)tq[a];
        }
        ev = sv / se;
    }
    o.lse_l = row_lse(l, A, row_max(l, A));
    o.lse_q = row_lse(qr, A, row_max(qr, A));
    o.V = 0.0;
    for (int64_t a = 0; a < A; ++a) o.V += exp((double)l[a] - o.lse_l) * (double)qr[a];
    o.qa = o.at >= 0 ? (double)qr[o.at] : (double)NAN;
    o.nlp = o.at >= 0 ? o.lse_l - (double)l[o.at] : (double)NAN;
    o.dq = o.qa - ((double)rew + gamma * ev);
    const double adv = o.qa - o.V;
    o.c = 1.0;
    o.dc = 0.0;
    if (mode == kCrrBinary) {
        o.c = adv > 0.0 ? 1.0 : 0.0;
    } else if (mode == kCrrExp) {
        const double e = exp(adv / beta);
        if (e < ub) {
            o.c = e;
            o.dc = e / beta;
        } else {
            o.c = e != e ? e : ub;  // torch's clamp keeps a NaN
        }
    }
    return o;
}

// Pass 1, one row per lane: the four row terms, summed in loss_sum.h's order.
__global__ __launch_bounds__(TPB) void crr_terms_kernel(
    const float* __restrict__ q, const float* __restrict__ logits,
    const int64_t* __restrict__ act, const float* __restrict__ t_logits,
    const float* __restrict__ t_q, const float* __restrict__ rew,
    const uint8_t* __restrict__ done, int64_t b, int64_t A, double gamma, int mode, double beta,
    double ub, double* __restrict__ partials, CrrLosses fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < b) {
        const CrrRow o = crr_row(q + r * A, logits + r * A, act[r], t_logits + r * A,
                                 t_q + r * A, rew[r], done[r], A, gamma, mode, beta, ub);
        term[0] = o.nlp;
        term[1] = o.c;
        term[2] = 0.5 * o.dq * o.dq;
        term[3] = o.lse_q - o.qa;
    }
    double s[4];
    block_sums<4>(term, s);
    losses_or_partials<4>(s, partials, fin);
}

// Pass 2, one row per lane, after the batch means nm = mean(nlp) and cm = mean(coef).  With
// p = softmax(l), V = sum_a p_a q_a, t the taken action and actor = nm * cm:
//   b * d actor / d l_a = -cm ([a == t] - p_a) + nm c' (-p_a (q_a - V))
//   b * d actor / d q_a = nm c' ([a == t] - p_a)
// c' = d coef / d adv of the row: c / beta in exp mode below the bound (the reference does not
// detach the coefficient), 0 otherwise.
__global__ __launch_bounds__(TPB) void crr_grad_kernel(
    const float* __restrict__ q, const float* __restrict__ logits,
    const int64_t* __restrict__ act, const float* __restrict__ t_logits,
    const float* __restrict__ t_q, const float* __restrict__ rew,
    const uint8_t* __restrict__ done, int64_t b, int64_t A, double gamma, int mode, double beta,
    double ub, double min_q_weight, const double* __restrict__ means,
    float* __restrict__ grad_q, float* __restrict__ grad_l) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    const float* qr = q + r * A;
    const float* l = logits + r * A;
    const CrrRow o = crr_row(qr, l, act[r], t_logits + r * A, t_q + r * A, rew[r], done[r], A,
                             gamma, mode, beta, ub);
    const double nm = means[0], cm = means[1], inv_b = 1.0 / (double)b;
    const double through = nm * o.dc;  // b * d actor / d adv of this row
    for (int64_t a = 0; a < A; ++a) {
        const double qv = (double)qr[a];
        const double p = exp((double)l[a] - o.lse_l);
        const double ind = a == o.at ? 1.0 : 0.0;
        double g_l = -cm * (ind - p);
        double g_q = (a == o.at ? o.dq : 0.0) + min_q_weight * (exp(qv - o.lse_q) - ind);
        if (o.dc != 0.0) {
            g_l -= through * p * (qv - o.V);
            g_q += through * (ind - p);
        }
        grad_l[r * A + a] = (float)(g_l * inv_b);
        grad_q[r * A + a] = (float)(g_q * inv_b);
    }
}

// The workgroup's sum of v in wave order, returned to every thread (dqn_dist.hip's block_sum:
// the same order, so the same bits).  red: NW doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    const double ws = wave_sum(v);
    __syncthreads();
    if ((t & (kWave - 1)) == 0) red[t / kWave] = ws;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < NW; ++i) s += red[i];
    return s;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// discrete_cql.py:57-76 for one row.  Dynamic LDS: 2 A doubles (the quantile means q_a, then
// p_a = softmax(q)_a) and the N target values.  Phase 1: wave w takes actions w, w + NW, ...
// with lanes over the quantiles.  Phase 2: wave 0 takes the logsumexp over the staged means.
// Phase 3: the thread that owns quantile i walks the N targets exactly as qr_loss_kernel does
// (same operations, same order, same block_sum), and writes the taken action's gradient entry;
// the workgroup writes the rest of the [A, N] tile in storage order.
__global__ __launch_bounds__(TPB) void cql_qr_loss_kernel(
    const float* __restrict__ curr, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ tau_hat,
    const float* __restrict__ weight, int64_t b, int64_t A, int64_t N, double min_q_weight,
    float* __restrict__ grad, float* __restrict__ prio, double* __restrict__ partials) {
    extern __shared__ double lds_d[];
    __shared__ double red[NW];
    __shared__ double s_lse;
    double* s_q = lds_d;
    double* s_p = lds_d + A;
    float* s_t = reinterpret_cast<float*>(lds_d + 2 * A);
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x;
    const int64_t a64 = act[r];
    const int64_t at = (a64 >= 0 && a64 < A) ? a64 : -1;
    const float* row = curr + r * A * N;
    float* g_row = grad + r * A * N;
    const double inv_n = 1.0 / (double)N;

    for (int64_t j = t; j < N; j += TPB) s_t[j] = returns[r * N + j];
    for (int64_t a = wv; a < A; a += NW) {
        const float* x = row + a * N;
        double acc = 0.0;
        for (int64_t n = lane; n < N; n += kWave) acc += (double)x[n];
        acc = wave_sum(acc);
        if (lane == 0) s_q[a] = acc * inv_n;
    }
    __syncthreads();
    if (wv == 0) {
        double m = -INFINITY;
        for (int64_t a = lane; a < A; a += kWave) m = fmax(m, s_q[a]);
        m = lse_shift(wave_max(m));
        double se = 0.0;
        for (int64_t a = lane; a < A; a += kWave) se += exp(s_q[a] - m);
        const double lse = m + log(wave_sum(se));
        for (int64_t a = lane; a < A; a += kWave) s_p[a] = exp(s_q[a] - lse);
        if (lane == 0) s_lse = lse;
    }
    __syncthreads();

    const double cscale = min_q_weight / ((double)b * (double)N);
    // every entry but the taken action's row: min_q_weight * p_a / (b N)
    const int64_t nel = A * N, lo = at * N, hi = lo + N;
    for (int64_t f = t; f < nel; f += TPB)
        if (at < 0 || f < lo || f >= hi)  // exact zeros at min_q_weight = 0, as qr_loss_kernel
            g_row[f] = (at < 0 || cscale == 0.0) ? 0.0f : (float)(s_p[f / N] * cscale);
    if (at < 0) {  // invalid action: NaN losses and priority, no gradient
        if (t == 0) {
            prio[r] = NAN;
            partials[r] = partials[b + r] = partials[2 * b + r] = (double)NAN;
        }
        return;
    }
    const double wr = weight ? (double)weight[r] : 1.0;
    const double gscale = wr / ((double)b * (double)N);
    const double c_taken = cscale == 0.0 ? 0.0 : (s_p[at] - 1.0) * cscale;
    const float* c_row = row + at * N;
    double hub = 0.0, pri = 0.0;
    for (int64_t i = t; i < N; i += TPB) {
        double hi_, g;
        qr_pair_walk(s_t, N, (double)c_row[i], (double)tau_hat[i], hi_, g, pri);
        hub += hi_;
        const double hg = -g * gscale;
        // a zero CQL part adds nothing, so that min_q_weight = 0 leaves qr_loss_kernel's bits
        g_row[lo + i] = (float)(c_taken == 0.0 ? hg : hg + c_taken);
    }
    const double hs = block_sum(hub, red) * inv_n;
    const double ps = block_sum(pri, red) * inv_n;
    if (t == 0) {
        prio[r] = (float)ps;
        partials[r] = hs * wr;
        partials[b + r] = s_lse;
        partials[2 * b + r] = s_q[at];
    }
}

// One wave over partials [3][b] (dist_fold_kernel's order per term): lane l sums entries
// l, l + 64, ... in index order, then the butterfly.  loss[0..3) = total, qr, cql.
__global__ __launch_bounds__(kWave) void cql_fold_kernel(const double* __restrict__ partials,
                                                         int64_t b, double min_q_weight,
                                                         float* __restrict__ loss) {
    double s[3];
    for (int k = 0; k < 3; ++k) {
        double v = 0.0;
        for (int64_t i = threadIdx.x; i < b; i += kWave) v += partials[k * b + i];
        s[k] = wave_sum(v);
    }
    if (threadIdx.x == 0) {
        const double qr = s[0] / (double)b;
        const double cql = s[1] / (double)b - s[2] / (double)b;
        loss[0] = (float)(qr + min_q_weight * cql);
        loss[1] = (float)qr;
        loss[2] = (float)cql;
    }
}

inline bool rows_ok(int64_t b, int64_t A) {
    return b >= 1 && b < ((int64_t)1 << 31) && A >= 1 && A < ((int64_t)1 << 31);
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_bcq_select(const float* q, const float* logits, double log_tau,
                               const float* q_eval, int paper, int64_t b, int64_t num_actions,
                               int64_t* act, float* val, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && (b == 0 || rows_ok(b, num_actions)),
                   "tsrl_bcq_select: need 0 <= b < 2^31 and 1 <= num_actions < 2^31");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(q && logits && act && (!q_eval == !val),
                   "tsrl_bcq_select: null pointer (q_eval and val come together)");
    hipLaunchKernelGGL(bcq_select_kernel, dim3((unsigned)loss_blocks(b)), dim3(TPB), 0,
                       as_stream(stream), q, logits, (float)log_tau, q_eval, paper, b,
                       num_actions, act, val);
    TSRL_LAUNCH_CHECK("tsrl_bcq_select");
    return 0;
}

extern "C" int tsrl_bcq_loss_fwd_bwd(const float* q, const float* logits, const int64_t* act,
                                     const float* returns, double weight_reg, int64_t b,
                                     int64_t num_actions, float* grad_q, float* grad_logits,
                                     double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(rows_ok(b, num_actions),
                   "tsrl_bcq_loss_fwd_bwd: need 1 <= b < 2^31 and 1 <= num_actions < 2^31");
    TSRL_CHECK_ARG(q && logits && act && returns && grad_q && grad_logits && loss,
                   "tsrl_bcq_loss_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const BcqLosses fin{(double)b, (double)b * (double)num_actions, weight_reg, loss};
    return launch_loss<3>("tsrl_bcq_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(bcq_loss_kernel, dim3(nblk), dim3(TPB), 0, st, q, logits, act,
                           returns, b, num_actions, weight_reg, grad_q, grad_logits, partials,
                           fin);
    });
}

extern "C" int tsrl_cql_qr_loss_fwd_bwd(const float* curr, const int64_t* act,
                                        const float* returns, const float* tau_hat,
                                        const float* weight, double min_q_weight, int64_t b,
                                        int64_t num_actions, int64_t n, float* grad, float* prio,
                                        double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) && num_actions >= 1 &&
                       num_actions <= kMaxA && n >= 1 && n <= kMaxN,
                   "tsrl_cql_qr_loss_fwd_bwd: need 1 <= b < 2^31, 1 <= num_actions <= %d, "
                   "1 <= n <= %d", (int)kMaxA, (int)kMaxN);
    TSRL_CHECK_ARG(curr && act && returns && tau_hat && grad && prio && partials && loss,
                   "tsrl_cql_qr_loss_fwd_bwd: null pointer");
    const size_t lds = (size_t)(2 * num_actions) * sizeof(double) + (size_t)n * sizeof(float);
    hipLaunchKernelGGL(cql_qr_loss_kernel, dim3((unsigned)b), dim3(TPB), lds, as_stream(stream),
                       curr, act, returns, tau_hat, weight, b, num_actions, n, min_q_weight,
                       grad, prio, partials);
    TSRL_LAUNCH_CHECK("tsrl_cql_qr_loss_fwd_bwd");
    hipLaunchKernelGGL(cql_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), partials, b,
                       min_q_weight, loss);
    TSRL_LAUNCH_CHECK("tsrl_cql_qr_loss_fwd_bwd (fold)");
    return 0;
}

extern "C" int tsrl_crr_loss_fwd_bwd(const float* q, const float* logits, const int64_t* act,
                                     const float* t_logits, const float* t_q, const float* rew,
                                     const uint8_t* done, double gamma, int mode, double beta,
                                     double ratio_upper_bound, double min_q_weight, int64_t b,
                                     int64_t num_actions, float* grad_q, float* grad_logits,
                                     double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(rows_ok(b, num_actions),
                   "tsrl_crr_loss_fwd_bwd: need 1 <= b < 2^31 and 1 <= num_actions < 2^31");
    TSRL_CHECK_ARG(mode >= kCrrExp && mode <= kCrrAll,
                   "tsrl_crr_loss_fwd_bwd: mode is 0 (exp), 1 (binary) or 2 (all)");
    TSRL_CHECK_ARG(q && logits && act && t_logits && t_q && rew && done && grad_q &&
                       grad_logits && loss,
                   "tsrl_crr_loss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(partials, "tsrl_crr_loss_fwd_bwd: partials is always needed");
    const hipStream_t st = as_stream(stream);
    double* means = partials;  // [2], then the block partials
    const CrrLosses fin{(double)b, min_q_weight, loss, means};
    const int rc = launch_loss<4>("tsrl_crr_loss_fwd_bwd", b, partials + 2, fin, st,
                                  [&](unsigned nblk) {
        hipLaunchKernelGGL(crr_terms_kernel, dim3(nblk), dim3(TPB), 0, st, q, logits, act,
                           t_logits, t_q, rew, done, b, num_actions, gamma, mode, beta,
                           ratio_upper_bound, partials + 2, fin);
    });
    if (rc != 0) return rc;
    hipLaunchKernelGGL(crr_grad_kernel, dim3((unsigned)loss_blocks(b)), dim3(TPB), 0, st, q,
                       logits, act, t_logits, t_q, rew, done, b, num_actions, gamma, mode, beta,
                       ratio_upper_bound, min_q_weight, means, grad_q, grad_logits);
    TSRL_LAUNCH_CHECK("tsrl_crr_loss_fwd_bwd (gradients)");
    return 0;
}
