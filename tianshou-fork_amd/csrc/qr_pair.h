// The quantile-regression pair walk of one current quantile against a row's N staged targets,
// defined once for qr_loss_kernel (dqn_dist.hip) and cql_qr_loss_kernel (offline.hip): the two
// promise the same bits, so they share the operations, their order and the contraction setting.
#pragma once
#include <stdint.h>

namespace tsrl {

// th: the current quantile, tau: its fraction, t[0..N): the targets.  hi = sum_j h(u_j) k_j,
// g = sum_j clamp(u_j, -1, 1) k_j with u_j = t[j] - th, h = smooth_l1 (beta 1) and
// k_j = |tau - 1{u_j <= 0}|; pri += sum_j h(u_j).
__device__ __forceinline__ void qr_pair_walk(const float* t, int64_t N, double th, double tau,
                                             double& hi, double& g, double& pri) {
    const double k_neg = fabs(tau - 1.0), k_pos = fabs(tau);
    hi = 0.0;
    g = 0.0;
    for (int64_t j = 0; j < N; ++j) {
        const double u = (double)t[j] - th;
        const double au = fabs(u);
        const double h = au < 1.0 ? 0.5 * u * u : au - 0.5;  // smooth_l1, beta 1
        const double k = u <= 0.0 ? k_neg : k_pos;
        hi += h * k;
        pri += h;
        g += fmin(fmax(u, -1.0), 1.0) * k;
    }
    if (hi != hi) {
        // Some u_j is NaN (a NaN target or quantile, inf - inf): h is NaN there, but fmin / fmax
        // above made the derivative -1.  torch's smooth_l1 backward keeps the NaN, so the sum
        // is taken again with it kept.  (hi is also NaN at inf * 0, a tau of exactly 0 or 1; the
        // second pass then gives what the first one gave.)
        g = 0.0;
        for (int64_t j = 0; j < N; ++j) {
            const double u = (double)t[j] - th;
            g += (u != u ? u : fmin(fmax(u, -1.0), 1.0)) * (u <= 0.0 ? k_neg : k_pos);
        }
    }
}

}  // namespace tsrl
