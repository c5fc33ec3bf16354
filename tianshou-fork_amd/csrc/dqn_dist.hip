// The distributional DQN family's small passes: C51Policy (tianshou/policy/modelfree/c51.py) and
// QRDQNPolicy (qrdqn.py).  The network's output is [b, A, N] (N atoms or quantiles per action).
//   dist_select:  compute_q_value (c51.py:71, qrdqn.py:73), the greedy action and the gather
//                 of that action's row (c51.py:74-81, qrdqn.py:59-68) in one launch;
//   c51_loss:     the categorical projection, the cross-entropy and its gradient
//                 (c51.py:82-102) without the [b, N, N] projection tensor;
//   qr_loss:      the pairwise quantile Huber loss, the priorities and the gradient
//                 (qrdqn.py:82-93) without its [b, N, N] tensors;
//   iqn_*:        IQNPolicy's siblings of dist_select and qr_loss for N online against M target
//                 quantiles at per-row fractions, read through strides, and the cosine
//                 embedding of ImplicitQuantileNetwork with its backward (further down);
//   fqf_*:        FQFPolicy's proposal forward (softmax, cumulative fractions, midpoints,
//                 entropy), its select (a template branch of iqn_select) and the fraction loss
//                 with its gradient to the proposal logits (at the end).
// One workgroup per batch row, lanes over the N atoms (a loop when N exceeds the workgroup):
// b is 32 to a few hundred, so the grid is b workgroups of one to four waves and the cost is
// launch latency.  Sums are f64 in a fixed order (lanes by xor butterfly, waves in wave order,
// rows in row order by the fold launch): bit-identical between runs, no atomics.
#include <float.h>

#include "loss_sum.h"
#include "tsrl_common.h"

namespace tsrl {
namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / kWave;
constexpr int64_t kMaxN = TSRL_DIST_MAX_N;  // the loss kernels stage 2 N floats in LDS (32 KiB)

// (v, a) replaces (best, arg) as the row's argmax: torch's rule (the first index of the
// maximum, the first NaN beats everything), for candidates met in any order.
__device__ __forceinline__ bool beats_at(float v, int64_t a, float best, int64_t arg) {
    const bool vn = v != v, bn = best != best;
    if (vn || bn) return vn && (!bn || a < arg);
    return v > best || (v == best && a < arg);
}

// The workgroup's sum of v in wave order, returned to every thread.  red: NW doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    const double ws = wave_sum(v);
    __syncthreads();  // red may still be read from an earlier call
    if ((t & (kWave - 1)) == 0) red[t / kWave] = ws;
    __syncthreads();
    const int nw = (blockDim.x + kWave - 1) / kWave;
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}

// Wave w takes actions w, w + NW, ...: lanes over the atoms, an f64 wave sum per action,
// rounded once to f32.  The waves' candidates meet in LDS; then the whole workgroup copies
// the chosen action's row.
__global__ __launch_bounds__(TPB) void dist_select_kernel(
    const float* __restrict__ sel, const float* __restrict__ eval, const float* __restrict__ w,
    int64_t A, int64_t N, float* __restrict__ q_out, int64_t* __restrict__ act_out,
    float* __restrict__ row_out) {
    __shared__ float s_best[NW];
    __shared__ int64_t s_arg[NW];
    __shared__ int64_t s_act;
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x;
    const float* row = sel + r * A * N;
    const double inv_n = 1.0 / (double)N;
    float best = 0.0f;
    int64_t arg = -1;
    for (int64_t a = wv; a < A; a += NW) {
        const float* x = row + a * N;
        double acc = 0.0;
        if (w) {
            for (int64_t n = lane; n < N; n += kWave) acc += (double)x[n] * (double)w[n];
        } else {
            for (int64_t n = lane; n < N; n += kWave) acc += (double)x[n];
        }
        acc = wave_sum(acc);
        const float q = (float)(w ? acc : acc * inv_n);
        if (q_out && lane == 0) q_out[r * A + a] = q;
        if (arg < 0 || beats_at(q, a, best, arg)) {
            best = q;
            arg = a;
        }
    }
    if (lane == 0) {
        s_best[wv] = best;
        s_arg[wv] = arg;
    }
    __syncthreads();
    if (t == 0) {
        best = s_best[0];
        arg = s_arg[0];  // wave 0 always holds action 0
        for (int i = 1; i < NW; ++i)
            if (s_arg[i] >= 0 && beats_at(s_best[i], s_arg[i], best, arg)) {
                best = s_best[i];
                arg = s_arg[i];
            }
        s_act = arg;
        if (act_out) act_out[r] = arg;
    }
    if (!row_out) return;
    __syncthreads();
    const float* src = (eval ? eval : sel) + (r * A + s_act) * N;
    for (int64_t n = t; n < N; n += TPB) row_out[r * N + n] = src[n];
}

// A row's loss term: the loss itself when the grid is one row, else that row's partial.
__device__ __forceinline__ void put_term(double term, double* __restrict__ partials,
                                         float* __restrict__ loss) {
    if (gridDim.x == 1)
        loss[0] = (float)term;
    else
        partials[blockIdx.x] = term;
}

// Zeros over the row's [A, N] gradient tile except the taken action's N entries, which their
// owners write.
__device__ __forceinline__ void zero_off_action(float* __restrict__ g_row, int64_t A, int64_t N,
                                                int64_t a_taken) {
    const int64_t nel = A * N, lo = a_taken * N, hi = lo + N;
    for (int64_t f = threadIdx.x; f < nel; f += blockDim.x)
        if (a_taken < 0 || f < lo || f >= hi) g_row[f] = 0.0f;
}

// c51.py:82-102 for one row.  LDS: the clamped returns and the next distribution, N floats
// each.  A thread owns atom i: its projected target t_i is a sum over the N staged pairs and
// never leaves registers.
__global__ __launch_bounds__(TPB) void c51_loss_kernel(
    const float* __restrict__ curr, const int64_t* __restrict__ act,
    const float* __restrict__ next, const float* __restrict__ returns,
    const float* __restrict__ support, const float* __restrict__ weight, int64_t b, int64_t A,
    int64_t N, float v_min, float v_max, double inv_dz, float* __restrict__ grad,
    float* __restrict__ ce, double* __restrict__ partials, float* __restrict__ loss) {
    extern __shared__ float lds[];
    __shared__ double red[NW];
    float* s_tz = lds;
    float* s_p = lds + N;
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t a64 = act[r];
    const int64_t a = (a64 >= 0 && a64 < A) ? a64 : -1;
    float* g_row = grad + r * A * N;
    zero_off_action(g_row, A, N, a);
    if (a < 0) {  // invalid action: NaN loss, no gradient
        if (t == 0) {
            ce[r] = NAN;
            put_term((double)NAN, partials, loss);
        }
        return;
    }
    for (int64_t j = t; j < N; j += blockDim.x) {
        const float x = returns[r * N + j];
        const bool nan = x != x;
        s_tz[j] = nan ? x : fminf(fmaxf(x, v_min), v_max);  // torch's clamp keeps a NaN
        // ... and so does its clamp(0, 1) of the projection weight: a NaN return's weight
        // towards every atom is NaN, and with it every t_i of the row, whatever next holds
        // there.  The fmin / fmax below drop a NaN, so it travels in the staged probability.
        s_p[j] = nan ? x : next[r * N + j];
    }
    __syncthreads();
    const double wr = weight ? (double)weight[r] : 1.0;
    const double gscale = wr / (double)b;
    const float* c_row = curr + (r * A + a) * N;
    double term = 0.0;
    for (int64_t i = t; i < N; i += blockDim.x) {
        const double z = (double)support[i];
        double ti = 0.0;
        for (int64_t j = 0; j < N; ++j) {
            double k = 1.0 - fabs((double)s_tz[j] - z) * inv_dz;
            k = fmin(fmax(k, 0.0), 1.0);
            ti += k * (double)s_p[j];
        }
        const double c = (double)c_row[i] + 1e-8;
        term -= ti * log(c);
        g_row[a * N + i] = (float)(-ti / c * gscale);
    }
    const double s = block_sum(term, red);
    if (t == 0) {
        ce[r] = (float)s;
        put_term(s * wr, partials, loss);
    }
}

// qrdqn.py:82-93 for one row.  LDS: the target row (returns), N floats.  A thread owns the
// current quantile i and walks the N targets.
__global__ __launch_bounds__(TPB) void qr_loss_kernel(
    const float* __restrict__ curr, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ tau_hat,
    const float* __restrict__ weight, int64_t b, int64_t A, int64_t N, float* __restrict__ grad,
    float* __restrict__ prio, double* __restrict__ partials, float* __restrict__ loss) {
    extern __shared__ float lds[];
    __shared__ double red[NW];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t a64 = act[r];
    const int64_t a = (a64 >= 0 && a64 < A) ? a64 : -1;
    float* g_row = grad + r * A * N;
    zero_off_action(g_row, A, N, a);
    if (a < 0) {
        if (t == 0) {
            prio[r] = NAN;
            put_term((double)NAN, partials, loss);
        }
        return;
    }
    for (int64_t j = t; j < N; j += blockDim.x) lds[j] = returns[r * N + j];
    __syncthreads();
    const double wr = weight ? (double)weight[r] : 1.0;
    const double inv_n = 1.0 / (double)N;
    const double gscale = wr / ((double)b * (double)N);
    const float* c_row = curr + (r * A + a) * N;
    double hub = 0.0, pri = 0.0;
    for (int64_t i = t; i < N; i += blockDim.x) {
        const double th = (double)c_row[i], tau = (double)tau_hat[i];
        const double k_neg = fabs(tau - 1.0), k_pos = fabs(tau);  // |tau - 1{u <= 0}|
        double hi = 0.0, g = 0.0;
        for (int64_t j = 0; j < N; ++j) {
            const double u = (double)lds[j] - th;
            const double au = fabs(u);
            const double h = au < 1.0 ? 0.5 * u * u : au - 0.5;  // smooth_l1, beta 1
            const double k = u <= 0.0 ? k_neg : k_pos;
            hi += h * k;
            pri += h;
            g += fmin(fmax(u, -1.0), 1.0) * k;
        }
        if (hi != hi) {
            // Some u_ij is NaN (a NaN target or quantile, inf - inf): h is NaN there, but fmin /
            // fmax above made the derivative -1.  torch's smooth_l1 backward keeps the NaN, so
            // this quantile's sum is taken again with it kept.  (hi is also NaN at inf * 0, a
            // tau_hat of exactly 0 or 1; the second pass then gives what the first one gave.)
            g = 0.0;
            for (int64_t j = 0; j < N; ++j) {
                const double u = (double)lds[j] - th;
                g += (u != u ? u : fmin(fmax(u, -1.0), 1.0)) * (u <= 0.0 ? k_neg : k_pos);
            }
        }
        hub += hi;
        g_row[a * N + i] = (float)(-g * gscale);
    }
    const double hs = block_sum(hub, red) * inv_n;
    const double ps = block_sum(pri, red) * inv_n;
    if (t == 0) {
        prio[r] = (float)ps;
        put_term(hs * wr, partials, loss);
    }
}

// One wave: lane l sums partials l, l + 64, ... in index order, then the butterfly.
__global__ __launch_bounds__(kWave) void dist_fold_kernel(const double* __restrict__ partials,
                                                          int64_t b, float* __restrict__ loss) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < b; i += kWave) s += partials[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = (float)(s / (double)b);
}

inline unsigned atom_threads(int64_t N) {
    const int64_t t = (N + kWave - 1) / kWave * kWave;
    return (unsigned)(t < TPB ? t : TPB);
}

// -- IQNPolicy (tianshou/policy/modelfree/iqn.py, utils/net/discrete.py:124-214) ------------------
// The network's head output is quantile-major, [b, N, A] seen as a [b, A, N] view: the select
// and loss kernels take the element strides of the A and N axes (sA, sN) and read either layout
// in place; a batch row is always A * N elements long.
constexpr int kMaxCos = TSRL_IQN_MAX_COSINES;  // cosines staged per fraction
constexpr int kFrac = 8;                       // fractions per workgroup: 8 * 256 doubles of LDS

// cos(pi (k + 1) tau) with the argument formed in f32 as CosineEmbeddingNetwork.forward forms
// it (an f32 arange times pi rounded to f32, then times tau); the cosine itself in f64.
__device__ __forceinline__ double iqn_cos(int k, float tau) {
    const float ipi = (float)(k + 1) * 3.14159274101257324f;
    const float arg = tau * ipi;
    return cos((double)arg);
}

// Workgroup (x, y): row x / nch, fractions (x % nch) * kFrac ..., features y * TPB ...  The
// fractions' cosines are staged once in LDS (f64); a thread owns feature d and walks W[d][:]
// once for its kFrac accumulators.  The k-sum is f64 FMA in index order starting from the bias;
// e and out are each rounded once from f64.
__global__ __launch_bounds__(TPB) void iqn_embed_fwd_kernel(
    const float* __restrict__ h, const float* __restrict__ taus, const float* __restrict__ W,
    const float* __restrict__ bias, int64_t N, int64_t D, int C, int64_t nch,
    float* __restrict__ e, float* __restrict__ out) {
    __shared__ double s_cos[kFrac][kMaxCos];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x / nch, n0 = (blockIdx.x % nch) * kFrac;
    const int nf = (int)(N - n0 < kFrac ? N - n0 : kFrac);
    for (int f = t; f < kFrac * C; f += TPB) {
        const int j = f / C, k = f - j * C;
        s_cos[j][k] = j < nf ? iqn_cos(k, taus[r * N + n0 + j]) : 0.0;
    }
    __syncthreads();
    const int64_t d = (int64_t)blockIdx.y * TPB + t;
    if (d >= D) return;
    double acc[kFrac];
    const double bd = (double)bias[d];
#pragma unroll
    for (int j = 0; j < kFrac; ++j) acc[j] = bd;
    const float* w = W + d * C;
    for (int k = 0; k < C; ++k) {
        const double wk = (double)w[k];
#pragma unroll
        for (int j = 0; j < kFrac; ++j) acc[j] = fma(s_cos[j][k], wk, acc[j]);
    }
    const double hd = (double)h[r * D + d];
#pragma unroll
    for (int j = 0; j < kFrac; ++j) {
        if (j < nf) {
            const double z = acc[j];
            const double ez = z > 0.0 ? z : (z != z ? z : 0.0);  // torch's relu keeps a NaN
            const int64_t o = (r * N + n0 + j) * D + d;
            e[o] = (float)ez;
            out[o] = (float)(hd * ez);
        }
    }
}

// Workgroup (x, y): row x, features y * TPB ...; a thread owns (row, d) and walks the N
// fractions in index order (g_h: an f64 sum rounded once).  The y == 0 workgroups also write
// the row's cosine features when asked.  gb_part (optional) gets the row's share of the bias
// gradient, sum_n g_z[(r,n)][d] in f64; iqn_gb_fold_kernel sums the rows in row order.
__global__ __launch_bounds__(TPB) void iqn_embed_bwd_kernel(
    const float* __restrict__ g_out, const float* __restrict__ e, const float* __restrict__ h,
    const float* __restrict__ taus, int64_t N, int64_t D, int C, float* __restrict__ g_h,
    float* __restrict__ g_z, float* __restrict__ cos_out, double* __restrict__ gb_part) {
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (cos_out && blockIdx.y == 0) {
        const int64_t nel = N * C;
        for (int64_t f = t; f < nel; f += TPB) {
            const int64_t n = f / C;
            cos_out[r * nel + f] = (float)iqn_cos((int)(f - n * C), taus[r * N + n]);
        }
    }
    const int64_t d = (int64_t)blockIdx.y * TPB + t;
    if (d >= D) return;
    const float hd = h[r * D + d];
    double s = 0.0, sb = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        const int64_t o = (r * N + n) * D + d;
        const float g = g_out[o], ev = e[o];
        s += (double)g * (double)ev;
        const bool dead = ev <= 0.0f;  // torch's threshold_backward: zero at z == 0
        g_z[o] = dead ? 0.0f : g * hd;
        sb += dead ? 0.0 : (double)g * (double)hd;
    }
    g_h[r * D + d] = (float)s;
    if (gb_part) gb_part[r * D + d] = sb;
}

// g_b[d] = sum_r gb_part[r][d], rows in row order, rounded once.
__global__ __launch_bounds__(TPB) void iqn_gb_fold_kernel(const double* __restrict__ gb_part,
                                                          int64_t B, int64_t D,
                                                          float* __restrict__ g_b) {
    const int64_t d = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int64_t r = 0; r < B; ++r) s += gb_part[r * D + d];
    g_b[d] = (float)s;
}

// dist_select_kernel with strides, a mean only, and an eval of its own column count M.
// FRAC (FQFPolicy, fqf.py:103-107): instead of the mean, the row's own weights taus[r][i + 1] -
// taus[r][i] (taus [b, N + 1]; the difference in f32 as torch forms it, product and sum f64).
template <bool FRAC>
__global__ __launch_bounds__(TPB) void iqn_select_kernel(
    const float* __restrict__ sel, int64_t sA, int64_t sN, const float* __restrict__ eval,
    int64_t eA, int64_t eM, const float* __restrict__ taus, int64_t A, int64_t N, int64_t M,
    float* __restrict__ q_out, int64_t* __restrict__ act_out, float* __restrict__ row_out) {
    __shared__ float s_best[NW];
    __shared__ int64_t s_arg[NW];
    __shared__ int64_t s_act;
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x;
    const float* row = sel + r * A * N;
    const double inv_n = 1.0 / (double)N;
    float best = 0.0f;
    int64_t arg = -1;
    for (int64_t a = wv; a < A; a += NW) {
        const float* x = row + a * sA;
        double acc = 0.0;
        if (FRAC) {
            const float* tr = taus + r * (N + 1);
            for (int64_t n = lane; n < N; n += kWave)
                acc += (double)(tr[n + 1] - tr[n]) * (double)x[n * sN];
        } else {
            for (int64_t n = lane; n < N; n += kWave) acc += (double)x[n * sN];
        }
        acc = wave_sum(acc);
        const float q = (float)(FRAC ? acc : acc * inv_n);
        if (q_out && lane == 0) q_out[r * A + a] = q;
        if (arg < 0 || beats_at(q, a, best, arg)) {
            best = q;
            arg = a;
        }
    }
    if (lane == 0) {
        s_best[wv] = best;
        s_arg[wv] = arg;
    }
    __syncthreads();
    if (t == 0) {
        best = s_best[0];
        arg = s_arg[0];  // wave 0 always holds action 0
        for (int i = 1; i < NW; ++i)
            if (s_arg[i] >= 0 && beats_at(s_best[i], s_arg[i], best, arg)) {
                best = s_best[i];
                arg = s_arg[i];
            }
        s_act = arg;
        if (act_out) act_out[r] = arg;
    }
    if (!row_out) return;
    __syncthreads();
    if (eval) {
        const float* src = eval + r * A * M + s_act * eA;
        for (int64_t n = t; n < M; n += TPB) row_out[r * M + n] = src[n * eM];
    } else {
        const float* src = row + s_act * sA;
        for (int64_t n = t; n < N; n += TPB) row_out[r * N + n] = src[n * sN];
    }
}

// iqn.py:93-108 for one row: qr_loss_kernel's pair walk with the row's own fractions and M
// targets (LDS: the M returns).  A thread owns the current quantile i; with M == N and
// taus[r] == tau_hat every operation is qr_loss_kernel's, in its order.
__global__ __launch_bounds__(TPB) void iqn_loss_kernel(
    const float* __restrict__ curr, int64_t sA, int64_t sN, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ taus,
    const float* __restrict__ weight, int64_t b, int64_t A, int64_t N, int64_t M,
    float* __restrict__ grad, float* __restrict__ prio, double* __restrict__ partials,
    float* __restrict__ loss) {
    extern __shared__ float lds[];
    __shared__ double red[NW];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int64_t a64 = act[r];
    const int64_t a = (a64 >= 0 && a64 < A) ? a64 : -1;
    float* g_row = grad + r * A * N;
    for (int64_t f = t; f < A * N; f += blockDim.x) {
        const int64_t fa = f / N;
        if (fa != a) g_row[fa * sA + (f - fa * N) * sN] = 0.0f;
    }
    if (a < 0) {
        if (t == 0) {
            prio[r] = NAN;
            put_term((double)NAN, partials, loss);
        }
        return;
    }
    for (int64_t j = t; j < M; j += blockDim.x) lds[j] = returns[r * M + j];
    __syncthreads();
    const double wr = weight ? (double)weight[r] : 1.0;
    const double inv_n = 1.0 / (double)N;
    const double gscale = wr / ((double)b * (double)N);
    const float* c_row = curr + r * A * N + a * sA;
    const float* tau_row = taus + r * N;
    double hub = 0.0, pri = 0.0;
    for (int64_t i = t; i < N; i += blockDim.x) {
        const double th = (double)c_row[i * sN], tau = (double)tau_row[i];
        const double k_neg = fabs(tau - 1.0), k_pos = fabs(tau);  // |tau - 1{u <= 0}|
        double hi = 0.0, g = 0.0;
        for (int64_t j = 0; j < M; ++j) {
            const double u = (double)lds[j] - th;
            const double au = fabs(u);
            const double h = au < 1.0 ? 0.5 * u * u : au - 0.5;  // smooth_l1, beta 1
            const double k = u <= 0.0 ? k_neg : k_pos;
            hi += h * k;
            pri += h;
            g += fmin(fmax(u, -1.0), 1.0) * k;
        }
        if (hi != hi) {
            // as qr_loss_kernel: a NaN u_ij keeps its NaN in the derivative; inf * 0 (a
            // fraction of exactly 0) takes the second pass and gets the first one's result
            g = 0.0;
            for (int64_t j = 0; j < M; ++j) {
                const double u = (double)lds[j] - th;
                g += (u != u ? u : fmin(fmax(u, -1.0), 1.0)) * (u <= 0.0 ? k_neg : k_pos);
            }
        }
        hub += hi;
        g_row[a * sA + i * sN] = (float)(-g * gscale);
    }
    const double hs = block_sum(hub, red) * inv_n;
    const double ps = block_sum(pri, red) * inv_n;
    if (t == 0) {
        prio[r] = (float)ps;
        put_term(hs * wr, partials, loss);
    }
}

// Either layout of a [b, A, N] view whose batch rows are A * N elements long.
inline bool row_strides_ok(int64_t sa, int64_t sn, int64_t A, int64_t N) {
    return (sa == N && sn == 1) || (sa == 1 && sn == A);
}

// -- FQFPolicy (tianshou/policy/modelfree/fqf.py, utils/net/discrete.py:217-316) -----------------
// A row's N values are cut into blockDim.x chunks of `per` consecutive elements, one per thread.
// The chunk sums are chained in index order by thread 0 and every thread then walks its own chunk
// in index order from its chain value, so with N <= blockDim.x the whole sum is in index order,
// and beyond that a prefix never exceeds the next one (a chunk's running sum ends at the value
// the chain carried on).  `tot` is the thread's chunk sum; chain: blockDim.x + 1 doubles.
// Forward: returns the sum of the chunks before this one, chain[blockDim.x] the row's sum.
__device__ __forceinline__ double chain_before(double tot, double* chain) {
    const int t = threadIdx.x, nt = blockDim.x;
    __syncthreads();  // chain may still be read from an earlier call
    chain[t] = tot;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int i = 0; i < nt; ++i) {
            const double c = chain[i];
            chain[i] = run;
            run += c;
        }
        chain[nt] = run;
    }
    __syncthreads();
    return chain[t];
}

// Backward: returns the sum of the chunks after this one.
__device__ __forceinline__ double chain_after(double tot, double* chain) {
    const int t = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    chain[t] = tot;
    __syncthreads();
    if (t == 0) {
        double run = 0.0;
        for (int i = nt - 1; i >= 0; --i) {
            const double c = chain[i];
            chain[i] = run;
            run += c;
        }
    }
    __syncthreads();
    return chain[t];
}

// discrete.py:241-249 for one row.  LDS: p as N doubles, then the rounded taus as N + 1 floats.
// max and logsumexp first, then logp_k = l_k - lse, p_k = exp(logp_k), the entropy, and the
// prefix sums of p by chain_before.  A NaN logit makes the maximum NaN and with it everything
// but taus[0].
__global__ __launch_bounds__(TPB) void fqf_propose_kernel(
    const float* __restrict__ logits, int64_t N, float* __restrict__ taus,
    float* __restrict__ tau_hats, float* __restrict__ entropies, float* __restrict__ logp_out) {
    extern __shared__ double lds_d[];
    __shared__ double red[NW];
    __shared__ double chain[TPB + 1];
    __shared__ float s_max[NW];
    double* p = lds_d;
    float* tau32 = reinterpret_cast<float*>(lds_d + N);
    const int t = threadIdx.x, nt = blockDim.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x;
    const float* l = logits + r * N;
    float m = -INFINITY;
    bool nan = false;
    for (int64_t k = t; k < N; k += nt) {
        const float v = l[k];
        nan |= v != v;
        m = fmaxf(m, v);
    }
    if (nan) m = NAN;
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(m, off, kWave);
        m = (m != m || o != o) ? NAN : fmaxf(m, o);
    }
    if (lane == 0) s_max[wv] = m;
    __syncthreads();
    m = s_max[0];
    for (int i = 1; i < (nt + kWave - 1) / kWave; ++i) {
        const float o = s_max[i];
        m = (m != m || o != o) ? NAN : fmaxf(m, o);
    }
    double se = 0.0;
    for (int64_t k = t; k < N; k += nt) se += exp((double)l[k] - (double)m);
    const double lse = (double)m + log(block_sum(se, red));
    double ent = 0.0;
    for (int64_t k = t; k < N; k += nt) {
        const double lp = (double)l[k] - lse;
        const double pk = exp(lp);
        p[k] = pk;
        logp_out[r * N + k] = (float)lp;
        // Categorical.entropy clamps logp at the lowest finite f32: a -inf logit gives 0 * that
        ent += pk * (lp < -(double)FLT_MAX ? -(double)FLT_MAX : lp);
    }
    const double es = block_sum(ent, red);  // its barriers also publish p
    if (t == 0) entropies[r] = (float)(-es);
    const int64_t per = (N + nt - 1) / nt;
    const int64_t lo = (int64_t)t * per, hi = lo + per < N ? lo + per : N;
    double tot = 0.0;
    for (int64_t k = lo; k < hi; ++k) tot += p[k];
    double run = chain_before(tot, chain);
    for (int64_t k = lo; k < hi; ++k) {
        tau32[k] = k == 0 ? 0.0f : (float)run;  // taus[0] is 0 whatever the row holds
        run += p[k];
    }
    if (t == 0) tau32[N] = (float)chain[nt];
    __syncthreads();
    float* tau_row = taus + r * (N + 1);
    for (int64_t k = t; k <= N; k += nt) tau_row[k] = tau32[k];
    for (int64_t k = t; k < N; k += nt) tau_hats[r * N + k] = (tau32[k] + tau32[k + 1]) / 2.0f;
}

// fqf.py:142-164 and its backward to the proposal logits for one row.  LDS: G as N floats (G[0]
// unused).  Thread i forms G_i in f32 as torch does; S_k, the suffix sums of G, by chain_after.
__global__ __launch_bounds__(TPB) void fqf_fraction_kernel(
    const float* __restrict__ curr, int64_t sA, int64_t sN, const float* __restrict__ qtau,
    int64_t tA, int64_t tN, const int64_t* __restrict__ act, const float* __restrict__ taus,
    const float* __restrict__ logp, const float* __restrict__ entropies, double ent_coef,
    int64_t b, int64_t A, int64_t N, float* __restrict__ g_logits,
    float* __restrict__ grad_taus_out, double* __restrict__ partials, MeanLosses<2> fin) {
    extern __shared__ float lds[];
    __shared__ double chain[TPB + 1];
    const int t = threadIdx.x, nt = blockDim.x;
    const int64_t r = blockIdx.x;
    const int64_t a = act[r];
    float* G = lds;
    double term[2] = {0.0, 0.0};
    double s[2];
    if (a < 0 || a >= A) {
        for (int64_t k = t; k < N; k += nt) g_logits[r * N + k] = NAN;
        if (grad_taus_out)
            for (int64_t i = t; i < N - 1; i += nt) grad_taus_out[r * (N - 1) + i] = NAN;
        if (t == 0) term[0] = term[1] = (double)NAN;
        block_sums<2>(term, s);
        losses_or_partials<2>(s, partials, fin);
        return;
    }
    const float* h = curr + r * A * N + a * sA;
    const float* q = qtau + r * A * (N - 1) + a * tA;
    const float* tau_row = taus + r * (N + 1);
    for (int64_t i = 1 + t; i < N; i += nt) {
        const float qi = q[(i - 1) * tN];
        const float left = i == 1 ? h[0] : q[(i - 2) * tN];
        const float right = i == N - 1 ? h[(N - 1) * sN] : q[i * tN];
        const float v1 = qi - h[(i - 1) * sN], v2 = qi - h[i * sN];
        const float g = (qi > left ? v1 : -v1) + (qi < right ? v2 : -v2);
        G[i] = g;
        if (grad_taus_out) grad_taus_out[r * (N - 1) + i - 1] = g;
        term[0] += (double)g * (double)tau_row[i];
    }
    if (t == 0) {
        G[0] = 0.0f;
        term[1] = (double)entropies[r];
    }
    block_sums<2>(term, s);  // its barrier also publishes G
    losses_or_partials<2>(s, partials, fin);
    // S_k = (1 / b) sum_{i > k} G_i over this thread's chunk of k, last to first
    const int64_t per = (N + nt - 1) / nt;
    const int64_t lo = (int64_t)t * per, hi = lo + per < N ? lo + per : N;
    double tot = 0.0;
    for (int64_t k = hi - 1; k >= lo; --k) tot += (double)G[k];
    // sum_{i > k} G_i = (the chunks after) + (this chunk's G after k); the chain is over G_k
    // themselves, so the walk adds G_k after using the sum
    const double after = chain_after(tot, chain);
    const double inv_b = 1.0 / (double)b;
    const float* lp_row = logp + r * N;
    double run = after, ps = 0.0;
    for (int64_t k = hi - 1; k >= lo; --k) {
        const double pk = exp((double)lp_row[k]);
        if (pk != 0.0) ps += pk * (run * inv_b);
        run += (double)G[k];
    }
    __shared__ double red[NW];
    const double sbar = block_sum(ps, red);
    const double H = (double)entropies[r], ec = ent_coef * inv_b;
    run = after;
    for (int64_t k = hi - 1; k >= lo; --k) {
        const double lp = (double)lp_row[k];
        const double pk = exp(lp);
        g_logits[r * N + k] =
            pk == 0.0 ? 0.0f : (float)(pk * (run * inv_b - sbar) + ec * pk * (lp + H));
        run += (double)G[k];
    }
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_dist_select(const float* sel, const float* eval, const float* w, int64_t b,
                                int64_t num_actions, int64_t n, float* q_out, int64_t* act_out,
                                float* row_out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1,
                   "tsrl_dist_select: need 0 <= b < 2^31, num_actions >= 1 and n >= 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(sel, "tsrl_dist_select: null pointer");
    hipLaunchKernelGGL(dist_select_kernel, dim3((unsigned)b), dim3(TPB), 0, as_stream(stream),
                       sel, eval, w, num_actions, n, q_out, act_out, row_out);
    TSRL_LAUNCH_CHECK("tsrl_dist_select");
    return 0;
}

extern "C" int tsrl_c51_loss_fwd_bwd(const float* curr, const int64_t* act, const float* next,
                                     const float* returns, const float* support,
                                     const float* weight, int64_t b, int64_t num_actions,
                                     int64_t n, float v_min, float v_max, double delta_z,
                                     float* grad, float* ce, double* partials, float* loss,
                                     void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 2 && n <= kMaxN,
                   "tsrl_c51_loss_fwd_bwd: need 1 <= b < 2^31, num_actions >= 1, 2 <= n <= %d",
                   (int)kMaxN);
    TSRL_CHECK_ARG(v_min < v_max && delta_z > 0.0,
                   "tsrl_c51_loss_fwd_bwd: need v_min < v_max and delta_z > 0");
    TSRL_CHECK_ARG(curr && act && next && returns && support && grad && ce && loss && (b == 1 || partials),
                   "tsrl_c51_loss_fwd_bwd: null pointer");
    hipLaunchKernelGGL(c51_loss_kernel, dim3((unsigned)b), dim3(atom_threads(n)),
                       (size_t)(2 * n) * sizeof(float), as_stream(stream), curr, act, next,
                       returns, support, weight, b, num_actions, n, v_min, v_max,
                       1.0 / delta_z, grad, ce, partials, loss);
    TSRL_LAUNCH_CHECK("tsrl_c51_loss_fwd_bwd");
    if (b > 1) {
        hipLaunchKernelGGL(dist_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                           partials, b, loss);
        TSRL_LAUNCH_CHECK("tsrl_c51_loss_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_qr_loss_fwd_bwd(const float* curr, const int64_t* act, const float* returns,
                                    const float* tau_hat, const float* weight, int64_t b,
                                    int64_t num_actions, int64_t n, float* grad, float* prio,
                                    double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1 && n <= kMaxN,
                   "tsrl_qr_loss_fwd_bwd: need 1 <= b < 2^31, num_actions >= 1, 1 <= n <= %d",
                   (int)kMaxN);
    TSRL_CHECK_ARG(curr && act && returns && tau_hat && grad && prio && loss && (b == 1 || partials),
                   "tsrl_qr_loss_fwd_bwd: null pointer");
    hipLaunchKernelGGL(qr_loss_kernel, dim3((unsigned)b), dim3(atom_threads(n)),
                       (size_t)n * sizeof(float), as_stream(stream), curr, act, returns, tau_hat,
                       weight, b, num_actions, n, grad, prio, partials, loss);
    TSRL_LAUNCH_CHECK("tsrl_qr_loss_fwd_bwd");
    if (b > 1) {
        hipLaunchKernelGGL(dist_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                           partials, b, loss);
        TSRL_LAUNCH_CHECK("tsrl_qr_loss_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_iqn_embed_fwd(const float* h, const float* taus, const float* w,
                                  const float* bias, int64_t b, int64_t n, int64_t d, int64_t c,
                                  float* e, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && n >= 1 && d >= 1 && c >= 1 && c <= kMaxCos,
                   "tsrl_iqn_embed_fwd: need b >= 0, n >= 1, d >= 1 and 1 <= c <= %d", kMaxCos);
    const int64_t nch = (n + kFrac - 1) / kFrac, ny = (d + TPB - 1) / TPB;
    TSRL_CHECK_ARG(b * nch < ((int64_t)1 << 31) && ny <= 65535,
                   "tsrl_iqn_embed_fwd: need b * ceil(n / %d) < 2^31 and d <= %d", kFrac,
                   65535 * TPB);
    if (b == 0) return 0;
    TSRL_CHECK_ARG(h && taus && w && bias && e && out, "tsrl_iqn_embed_fwd: null pointer");
    hipLaunchKernelGGL(iqn_embed_fwd_kernel, dim3((unsigned)(b * nch), (unsigned)ny), dim3(TPB),
                       0, as_stream(stream), h, taus, w, bias, n, d, (int)c, nch, e, out);
    TSRL_LAUNCH_CHECK("tsrl_iqn_embed_fwd");
    return 0;
}

extern "C" int tsrl_iqn_embed_bwd(const float* g_out, const float* e, const float* h,
                                  const float* taus, int64_t b, int64_t n, int64_t d, int64_t c,
                                  float* g_h, float* g_z, float* cos_out, double* gb_part,
                                  float* g_b, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && n >= 1 && d >= 1 && c >= 1 &&
                       (d + TPB - 1) / TPB <= 65535,
                   "tsrl_iqn_embed_bwd: need 0 <= b < 2^31, n >= 1, 1 <= d <= %d and c >= 1",
                   65535 * TPB);
    if (b == 0) return 0;
    TSRL_CHECK_ARG(g_out && e && h && g_h && g_z && (!cos_out || taus) && (!g_b == !gb_part),
                   "tsrl_iqn_embed_bwd: null pointer (cos_out needs taus, g_b needs gb_part)");
    hipLaunchKernelGGL(iqn_embed_bwd_kernel, dim3((unsigned)b, (unsigned)((d + TPB - 1) / TPB)),
                       dim3(TPB), 0, as_stream(stream), g_out, e, h, taus, n, d, (int)c, g_h,
                       g_z, cos_out, gb_part);
    TSRL_LAUNCH_CHECK("tsrl_iqn_embed_bwd");
    if (g_b) {
        hipLaunchKernelGGL(iqn_gb_fold_kernel, dim3((unsigned)((d + TPB - 1) / TPB)), dim3(TPB), 0,
                           as_stream(stream), gb_part, b, d, g_b);
        TSRL_LAUNCH_CHECK("tsrl_iqn_embed_bwd (bias fold)");
    }
    return 0;
}

extern "C" int tsrl_iqn_select(const float* sel, int64_t sel_sa, int64_t sel_sn,
                               const float* eval, int64_t eval_sa, int64_t eval_sm, int64_t b,
                               int64_t num_actions, int64_t n, int64_t m, float* q_out,
                               int64_t* act_out, float* row_out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1,
                   "tsrl_iqn_select: need 0 <= b < 2^31, num_actions >= 1 and n >= 1");
    TSRL_CHECK_ARG(row_strides_ok(sel_sa, sel_sn, num_actions, n),
                   "tsrl_iqn_select: sel strides (%lld, %lld) are neither [b, A, N] nor the "
                   "[b, N, A] view", (long long)sel_sa, (long long)sel_sn);
    TSRL_CHECK_ARG(!eval || (m >= 1 && row_strides_ok(eval_sa, eval_sm, num_actions, m)),
                   "tsrl_iqn_select: eval needs m >= 1 and strides of [b, A, M] or its "
                   "[b, M, A] view");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(sel, "tsrl_iqn_select: null pointer");
    hipLaunchKernelGGL(iqn_select_kernel<false>, dim3((unsigned)b), dim3(TPB), 0,
                       as_stream(stream), sel, sel_sa, sel_sn, eval, eval_sa, eval_sm,
                       (const float*)nullptr, num_actions, n, m, q_out, act_out, row_out);
    TSRL_LAUNCH_CHECK("tsrl_iqn_select");
    return 0;
}

extern "C" int tsrl_iqn_loss_fwd_bwd(const float* curr, int64_t sa, int64_t sn,
                                     const int64_t* act, const float* returns, const float* taus,
                                     const float* weight, int64_t b, int64_t num_actions,
                                     int64_t n, int64_t m, float* grad, float* prio,
                                     double* partials, float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 2 && n <= kMaxN &&
                       m >= 2 && m <= kMaxN,
                   "tsrl_iqn_loss_fwd_bwd: need 1 <= b < 2^31, num_actions >= 1, 2 <= n, m <= %d",
                   (int)kMaxN);
    TSRL_CHECK_ARG(row_strides_ok(sa, sn, num_actions, n),
                   "tsrl_iqn_loss_fwd_bwd: strides (%lld, %lld) are neither [b, A, N] nor the "
                   "[b, N, A] view", (long long)sa, (long long)sn);
    TSRL_CHECK_ARG(curr && act && returns && taus && grad && prio && loss && (b == 1 || partials),
                   "tsrl_iqn_loss_fwd_bwd: null pointer");
    hipLaunchKernelGGL(iqn_loss_kernel, dim3((unsigned)b), dim3(atom_threads(n)),
                       (size_t)m * sizeof(float), as_stream(stream), curr, sa, sn, act, returns,
                       taus, weight, b, num_actions, n, m, grad, prio, partials, loss);
    TSRL_LAUNCH_CHECK("tsrl_iqn_loss_fwd_bwd");
    if (b > 1) {
        hipLaunchKernelGGL(dist_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream),
                           partials, b, loss);
        TSRL_LAUNCH_CHECK("tsrl_iqn_loss_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_fqf_propose_fwd(const float* logits, int64_t b, int64_t n, float* taus,
                                    float* tau_hats, float* entropies, float* logp,
                                    void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && n >= 2 && n <= kMaxN,
                   "tsrl_fqf_propose_fwd: need 0 <= b < 2^31 and 2 <= n <= %d", (int)kMaxN);
    if (b == 0) return 0;
    TSRL_CHECK_ARG(logits && taus && tau_hats && entropies && logp,
                   "tsrl_fqf_propose_fwd: null pointer");
    hipLaunchKernelGGL(fqf_propose_kernel, dim3((unsigned)b), dim3(atom_threads(n)),
                       (size_t)n * sizeof(double) + (size_t)(n + 1) * sizeof(float),
                       as_stream(stream), logits, n, taus, tau_hats, entropies, logp);
    TSRL_LAUNCH_CHECK("tsrl_fqf_propose_fwd");
    return 0;
}

extern "C" int tsrl_fqf_select(const float* sel, int64_t sel_sa, int64_t sel_sn,
                               const float* eval, int64_t eval_sa, int64_t eval_sm,
                               const float* taus, int64_t b, int64_t num_actions, int64_t n,
                               float* q_out, int64_t* act_out, float* row_out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1,
                   "tsrl_fqf_select: need 0 <= b < 2^31, num_actions >= 1 and n >= 1");
    TSRL_CHECK_ARG(row_strides_ok(sel_sa, sel_sn, num_actions, n),
                   "tsrl_fqf_select: sel strides (%lld, %lld) are neither [b, A, N] nor the "
                   "[b, N, A] view", (long long)sel_sa, (long long)sel_sn);
    TSRL_CHECK_ARG(!eval || row_strides_ok(eval_sa, eval_sm, num_actions, n),
                   "tsrl_fqf_select: eval needs the strides of [b, A, N] or its [b, N, A] view");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(sel && taus, "tsrl_fqf_select: null pointer");
    hipLaunchKernelGGL(iqn_select_kernel<true>, dim3((unsigned)b), dim3(TPB), 0,
                       as_stream(stream), sel, sel_sa, sel_sn, eval, eval_sa, eval_sm, taus,
                       num_actions, n, n, q_out, act_out, row_out);
    TSRL_LAUNCH_CHECK("tsrl_fqf_select");
    return 0;
}

extern "C" int tsrl_fqf_fraction_loss_fwd_bwd(const float* curr, int64_t sa, int64_t sn,
                                              const float* qtau, int64_t ta, int64_t tn,
                                              const int64_t* act, const float* taus,
                                              const float* logp, const float* entropies,
                                              double ent_coef, int64_t b, int64_t num_actions,
                                              int64_t n, float* g_logits, float* grad_taus_out,
                                              double* partials, float* losses, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 2 && n <= kMaxN,
                   "tsrl_fqf_fraction_loss_fwd_bwd: need 1 <= b < 2^31, num_actions >= 1, "
                   "2 <= n <= %d", (int)kMaxN);
    TSRL_CHECK_ARG(row_strides_ok(sa, sn, num_actions, n) &&
                       row_strides_ok(ta, tn, num_actions, n - 1),
                   "tsrl_fqf_fraction_loss_fwd_bwd: strides (%lld, %lld) of curr or (%lld, %lld) "
                   "of qtau are neither [b, A, .] nor the [b, ., A] view", (long long)sa,
                   (long long)sn, (long long)ta, (long long)tn);
    TSRL_CHECK_ARG(curr && qtau && act && taus && logp && entropies && g_logits && losses &&
                       (b == 1 || partials),
                   "tsrl_fqf_fraction_loss_fwd_bwd: null pointer");
    const MeanLosses<2> fin{(double)b, 1.0f, losses, nullptr};
    hipLaunchKernelGGL(fqf_fraction_kernel, dim3((unsigned)b), dim3(TPB),
                       (size_t)n * sizeof(float), as_stream(stream), curr, sa, sn, qtau, ta, tn,
                       act, taus, logp, entropies, ent_coef, b, num_actions, n, g_logits,
                       grad_taus_out, partials, fin);
    TSRL_LAUNCH_CHECK("tsrl_fqf_fraction_loss_fwd_bwd");
    if (b > 1) {
        hipLaunchKernelGGL((loss_fold_kernel<2, MeanLosses<2>>), dim3(1), dim3(kWave), 0,
                           as_stream(stream), partials, b, fin);
        TSRL_LAUNCH_CHECK("tsrl_fqf_fraction_loss_fwd_bwd (fold)");
    }
    return 0;
}
