// DQNPolicy's three small passes (tianshou/policy/modelfree/dqn.py): the bootstrap value of
// _target_q after the two forwards (:85-96), learn()'s TD loss with its gradient (:172-185),
// and exploration_noise's epsilon-greedy overwrite (:190-203).  A DQN minibatch is 32 to a few
// hundred rows of <= 18 actions, so every kernel is one row per lane with a loop over the
// actions: the work is launch latency, and each kernel replaces 3-10 torch launches.
#include "loss_sum.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;

// torch's max / argmax over a row: the first index of the maximum, a NaN beats every number
// (the first NaN wins).
__device__ __forceinline__ bool beats(float v, float best) {
    return v > best || (v != v && best == best);
}

__global__ __launch_bounds__(TPB) void target_q_kernel(const float* __restrict__ q_sel,
                                                       const float* __restrict__ q_eval,
                                                       int64_t b, int64_t A, int is_double,
                                                       float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    const float* s = (is_double ? q_sel : q_eval) + r * A;
    float best = s[0];
    int64_t arg = 0;
    for (int64_t a = 1; a < A; ++a) {
        const float v = s[a];
        if (beats(v, best)) {
            best = v;
            arg = a;
        }
    }
    out[r] = is_double ? q_eval[r * A + arg] : best;
}

// One workgroup = 256 rows.  Each lane computes its row's TD error, loss term and the one
// non-zero gradient entry; the [rows, A] gradient tile is then written by the whole workgroup
// in storage order (zeros off the taken action), after block_sums' barrier.  The loss terms are
// summed in loss_sum.h's fixed order.
__global__ __launch_bounds__(TPB) void td_fwd_bwd_kernel(
    const float* __restrict__ q, const int64_t* __restrict__ act,
    const float* __restrict__ returns, const float* __restrict__ weight, int64_t b, int64_t A,
    int huber, float inv_b, float* __restrict__ grad_q, float* __restrict__ td_error,
    double* __restrict__ partials, MeanLosses<1> fin) {
    __shared__ float s_g[TPB];
    __shared__ int s_a[TPB];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * TPB;
    const int nrows = (int)min((int64_t)TPB, b - r0);
    double term[1] = {0.0};
    float g = 0.0f;
    int a = -1;
    if (t < nrows) {
        const int64_t r = r0 + t;
        const int64_t a64 = act[r];
        a = (a64 >= 0 && a64 < A) ? (int)a64 : -1;  // invalid action -> NaN loss, no gradient
        const float qa = a >= 0 ? q[r * A + a] : NAN;
        const float td = returns[r] - qa;
        td_error[r] = td;
        if (huber) {  // torch huber_loss, delta 1, on x = q_a - returns = -td
            const float ax = fabsf(td);
            term[0] = (double)(ax < 1.0f ? 0.5f * td * td : ax - 0.5f);
            g = (td >= 1.0f ? -1.0f : td <= -1.0f ? 1.0f : -td) * inv_b;
        } else {
            const float w = weight ? weight[r] : 1.0f;
            term[0] = (double)(td * td * w);
            g = -2.0f * td * w * inv_b;
        }
    }
    s_g[t] = g;
    s_a[t] = a;
    double s[1];
    block_sums<1>(term, s);
    const int64_t nel = (int64_t)nrows * A;
    float* g_blk = grad_q + r0 * A;
    for (int64_t f = t; f < nel; f += TPB) {
        const int row = (int)(f / A);
        const int col = (int)(f - (int64_t)row * A);
        g_blk[f] = col == s_a[row] ? s_g[row] : 0.0f;
    }
    losses_or_partials<1>(s, partials, fin);
}

// NumPy's f64 arithmetic: q = u_act + mask, the first index of the maximum.
__global__ __launch_bounds__(TPB) void eps_greedy_kernel(int64_t* __restrict__ act,
                                                         const double* __restrict__ u_row,
                                                         const double* __restrict__ u_act,
                                                         const uint8_t* __restrict__ mask,
                                                         double eps, int64_t n, int64_t A) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    if (!(u_row[r] < eps)) return;
    const double* u = u_act + r * A;
    const uint8_t* m = mask ? mask + r * A : nullptr;
    double best = u[0] + (m ? (double)m[0] : 0.0);
    int64_t arg = 0;
    for (int64_t a = 1; a < A; ++a) {
        const double v = u[a] + (m ? (double)m[a] : 0.0);
        if (v > best) {
            best = v;
            arg = a;
        }
    }
    act[r] = arg;
}

inline unsigned row_blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_dqn_target_q(const float* q_sel, const float* q_eval, int64_t b,
                                 int64_t num_actions, int is_double, float* out,
                                 void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) * TPB && num_actions >= 1,
                   "tsrl_dqn_target_q: need b >= 0 and num_actions >= 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(q_eval && out && (!is_double || q_sel), "tsrl_dqn_target_q: null pointer");
    hipLaunchKernelGGL(target_q_kernel, dim3(row_blocks(b)), dim3(TPB), 0, as_stream(stream),
                       q_sel, q_eval, b, num_actions, is_double, out);
    TSRL_LAUNCH_CHECK("tsrl_dqn_target_q");
    return 0;
}

extern "C" int64_t tsrl_dqn_num_partials(int64_t b) { return loss_blocks(b); }

extern "C" int tsrl_dqn_td_fwd_bwd(const float* q, const int64_t* act, const float* returns,
                                   const float* weight, int64_t b, int64_t num_actions,
                                   int huber, float* grad_q, float* td_error, double* partials,
                                   float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB && num_actions >= 1,
                   "tsrl_dqn_td_fwd_bwd: need b >= 1 and num_actions >= 1");
    TSRL_CHECK_ARG(q && act && returns && grad_q && td_error && loss,
                   "tsrl_dqn_td_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const MeanLosses<1> fin{(double)b, 1.0f, loss, nullptr};
    return launch_loss<1>("tsrl_dqn_td_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(td_fwd_bwd_kernel, dim3(nblk), dim3(TPB), 0, st, q, act, returns,
                           weight, b, num_actions, huber, 1.0f / (float)b, grad_q, td_error,
                           partials, fin);
    });
}

extern "C" int tsrl_eps_greedy(int64_t* act, const double* u_row, const double* u_act,
                               const uint8_t* mask, double eps, int64_t n, int64_t num_actions,
                               void* stream) {
    TSRL_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) * TPB && num_actions >= 1,
                   "tsrl_eps_greedy: need n >= 0 and num_actions >= 1");
    if (n == 0) return 0;
    TSRL_CHECK_ARG(act && u_row && u_act, "tsrl_eps_greedy: null pointer");
    hipLaunchKernelGGL(eps_greedy_kernel, dim3(row_blocks(n)), dim3(TPB), 0, as_stream(stream),
                       act, u_row, u_act, mask, eps, n, num_actions);
    TSRL_LAUNCH_CHECK("tsrl_eps_greedy");
    return 0;
}
