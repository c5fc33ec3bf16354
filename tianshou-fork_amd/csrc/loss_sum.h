// The f64 batch reduction of the off-policy loss kernels, defined once for dqn.hip, ddpg.hip,
// sac.hip, dsac.hip and redq.hip.  A kernel's NK per-row loss terms are summed in a fixed order:
// lanes by xor butterfly, the four waves in wave order, the workgroups in block order.  One
// workgroup finishes the losses itself; more write partials[k][blockIdx.x] and loss_fold_kernel
// sums them and runs the same finish.  The order, and every division and cast in the two finish
// functors, are part of the numerical contract (tests/test_gpu_loss_sum.py restates them).
#pragma once
#include "tsrl_common.h"

namespace tsrl {

constexpr int kLossTPB = 256;  // one workgroup = 256 rows
constexpr int kLossWaves = kLossTPB / kWave;

// Workgroups of a loss kernel over b rows = the partials per loss term.
inline int64_t loss_blocks(int64_t b) { return b > 0 ? (b + kLossTPB - 1) / kLossTPB : 0; }

// torch.min(a, b): a NaN on either side is handed through.
__device__ __forceinline__ float min_nan(float a, float b) {
    return a != a ? a : (b != b ? b : (b < a ? b : a));
}

// The workgroup's sums: lane 0 gets s[0..NK).  Every lane passes the one barrier in here, so
// shared memory written before the call may be read by any lane after it.
template <int NK>
__device__ __forceinline__ void block_sums(const double* term, double* s) {
    __shared__ double red[NK][kLossWaves];
    const int t = threadIdx.x;
    for (int k = 0; k < NK; ++k) {
        const double ws = wave_sum(term[k]);
        if ((t & (kWave - 1)) == 0) red[k][t / kWave] = ws;
    }
    __syncthreads();
    if (t == 0) {
        for (int k = 0; k < NK; ++k) {
            s[k] = 0.0;
            for (int i = 0; i < kLossWaves; ++i) s[k] += red[k][i];
        }
    }
}

// Lane 0, after block_sums: finish the losses, or hand the sums to loss_fold_kernel.
template <int NK, class Finish>
__device__ __forceinline__ void losses_or_partials(const double* s,
                                                   double* __restrict__ partials, Finish fin) {
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) {
        fin(s);
    } else {
        for (int k = 0; k < NK; ++k) partials[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
    }
}

// loss[k] = sign * s[k] / n, total (optional) = sign * the sum of those quotients.
template <int NK>
struct MeanLosses {
    double n;
    float sign;
    float* loss;
    float* total;
    __device__ void operator()(const double* s) const {
        double tot = 0.0;
        for (int k = 0; k < NK; ++k) {
            const double l = s[k] / n;
            loss[k] = sign * (float)l;
            tot += l;
        }
        if (total) total[0] = sign * (float)tot;
    }
};

// An actor loss with SAC's temperature loss: loss[0] = sign0 * s[0] / b; with log_alpha,
// m = s[1] / b, loss[1] = -log_alpha * m and g_log_alpha = -m.
struct ActorAlphaLosses {
    double b, sign0;
    const float* log_alpha;
    float* loss;
    float* g_log_alpha;
    __device__ void operator()(const double* s) const {
        loss[0] = (float)(sign0 * (s[0] / b));
        if (log_alpha) {
            const double m = s[1] / b;
            loss[1] = (float)(-(double)log_alpha[0] * m);
            g_log_alpha[0] = (float)(-m);
        }
    }
};

// partials [NK][nblk] -> the finished losses.
template <int NK, class Finish>
__global__ void loss_fold_kernel(const double* __restrict__ partials, int64_t nblk, Finish fin) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s[NK];
        for (int k = 0; k < NK; ++k) {
            s[k] = 0.0;
            for (int64_t i = 0; i < nblk; ++i) s[k] += partials[(int64_t)k * nblk + i];
        }
        fin(s);
    }
}

// The host side of a loss kernel over b rows: launch(nblk) starts the kernel on nblk workgroups
// of kLossTPB threads, with `partials` and `fin` among its arguments.
template <int NK, class Finish, class Launch>
inline int launch_loss(const char* name, int64_t b, const double* partials, Finish fin,
                       hipStream_t stream, Launch launch) {
    const int64_t nblk = loss_blocks(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "%s: b > %d needs partials", name, kLossTPB);
    launch((unsigned)nblk);
    TSRL_LAUNCH_CHECK(name);
    if (nblk > 1) {
        hipLaunchKernelGGL((loss_fold_kernel<NK, Finish>), dim3(1), dim3(kWave), 0, stream,
                           partials, nblk, fin);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            set_error("%s (fold): launch failed: %s", name, hipGetErrorString(e));
            return (int)e;
        }
    }
    return 0;
}

}  // namespace tsrl
