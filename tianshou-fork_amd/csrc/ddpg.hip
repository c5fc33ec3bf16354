// DDPGPolicy / TD3Policy (tianshou/policy/modelfree/ddpg.py, td3.py): the glue around the
// actor and critic forwards.  A minibatch is a few hundred rows of <= 17 actions and a network
// a few hundred thousand parameters, so every pass here is launch latency: each kernel replaces
// a chain of torch launches (the Polyak update alone is three per parameter tensor).
//   soft_update_kernel   sync_weight (ddpg.py:117-120, td3.py:93-96) over up to four networks
//   td3_smooth_kernel    target policy smoothing (td3.py:100-104)
//   q_mse_kernel         _mse_optimizer's TD error, loss and gradient (ddpg.py:173-178), one or
//                        two critics
//   neg_mean_kernel      the actor loss -Q.mean() (ddpg.py:189) and its constant gradient
//   act_noise_kernel     exploration_noise (ddpg.py:202) over the caller's NumPy draws
#include "tsrl_common.h"

namespace tsrl {
namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / kWave;
constexpr int kMaxSeg = 4;
constexpr unsigned kMaxBlocks = 1024;

struct Seg {
    float* t;
    const float* s;
    int64_t n;
};
struct Segs {
    Seg seg[kMaxSeg];
};

// torch's fp32 `tau * s + (1 - tau) * t`: two rounded products and a rounded sum, no FMA.
__device__ __forceinline__ float polyak(float s, float t, float tau, float omt) {
#pragma clang fp contract(off)
    const float a = tau * s;
    const float b = omt * t;
    return a + b;
}

// blockIdx.y = segment.  A segment is a slice of a flat buffer and may start at any 4-byte
// offset: when target and source are misaligned alike, the elements up to the first 16-byte
// boundary and those after the last whole float4 go one per lane and the body as float4;
// otherwise every element goes one per lane.
__global__ __launch_bounds__(TPB) void soft_update_kernel(Segs segs, float tau, float omt) {
    const Seg sg = segs.seg[blockIdx.y];
    float* __restrict__ t = sg.t;
    const float* __restrict__ s = sg.s;
    const int64_t n = sg.n;
    const int64_t tid = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * TPB;
    const uintptr_t mt = reinterpret_cast<uintptr_t>(t) & 15u;
    const uintptr_t ms = reinterpret_cast<uintptr_t>(s) & 15u;
    int64_t head = n, nvec = 0;
    if (mt == ms) {
        head = min(n, (int64_t)(((16u - mt) & 15u) / 4u));
        nvec = (n - head) / 4;
    }
    float4* t4 = reinterpret_cast<float4*>(t + head);
    const float4* s4 = reinterpret_cast<const float4*>(s + head);
    for (int64_t i = tid; i < nvec; i += stride) {
        const float4 a = s4[i];
        float4 b = t4[i];
        b.x = polyak(a.x, b.x, tau, omt);
        b.y = polyak(a.y, b.y, tau, omt);
        b.z = polyak(a.z, b.z, tau, omt);
        b.w = polyak(a.w, b.w, tau, omt);
        t4[i] = b;
    }
    const int64_t body_end = head + 4 * nvec;
    const int64_t nscalar = head + (n - body_end);
    for (int64_t i = tid; i < nscalar; i += stride) {
        const int64_t j = i < head ? i : body_end + (i - head);
        t[j] = polyak(s[j], t[j], tau, omt);
    }
}

// out = a + clamp(noise * sigma, -c, c); torch.clamp hands a NaN through.
__global__ __launch_bounds__(TPB) void td3_smooth_kernel(const float* a,
                                                         const float* __restrict__ noise,
                                                         float sigma, float c, int64_t n,
                                                         float* out) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    float e = noise[i] * sigma;
    if (c > 0.0f && e == e) e = e < -c ? -c : (e > c ? c : e);
    out[i] = a[i] + e;
}

// One workgroup = 256 rows of every critic.  The loss terms are summed in f64 in a fixed order:
// lanes by xor butterfly, the four waves in wave order, the workgroups in block order (by this
// kernel when there is one workgroup, else by q_fold_kernel).
__device__ __forceinline__ void finish_losses(const double* s, int nk, int64_t b, float sign,
                                              float* loss, float* total) {
    double tot = 0.0;
    for (int k = 0; k < nk; ++k) {
        const double l = s[k] / (double)b;
        loss[k] = sign * (float)l;
        tot += l;
    }
    if (total) total[0] = sign * (float)tot;
}

__global__ __launch_bounds__(TPB) void q_mse_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ returns, const float* __restrict__ weight, int64_t b, float inv_b,
    float* __restrict__ grad1, float* __restrict__ grad2, float* __restrict__ td_out,
    double* __restrict__ partials, float* __restrict__ loss, float* __restrict__ total) {
#pragma clang fp contract(off)
    __shared__ double red[2][NW];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * TPB + t;
    const int nk = q2 ? 2 : 1;
    double term[2] = {0.0, 0.0};
    if (r < b) {
        const float ret = returns[r];
        const float w = weight ? weight[r] : 1.0f;
        const float td1 = q1[r] - ret;
        term[0] = (double)(td1 * td1 * w);
        grad1[r] = 2.0f * td1 * w * inv_b;
        float row = td1;
        if (q2) {
            const float td2 = q2[r] - ret;
            term[1] = (double)(td2 * td2 * w);
            grad2[r] = 2.0f * td2 * w * inv_b;
            row = (td1 + td2) / 2.0f;
        }
        td_out[r] = row;
    }
    for (int k = 0; k < nk; ++k) {
        const double ws = wave_sum(term[k]);
        if ((t & (kWave - 1)) == 0) red[k][t / kWave] = ws;
    }
    __syncthreads();
    if (t == 0) {
        double s[2] = {0.0, 0.0};
        for (int k = 0; k < nk; ++k)
            for (int i = 0; i < NW; ++i) s[k] += red[k][i];
        if (gridDim.x == 1) {
            finish_losses(s, nk, b, 1.0f, loss, total);
        } else {
            for (int k = 0; k < nk; ++k) partials[(int64_t)k * gridDim.x + blockIdx.x] = s[k];
        }
    }
}

__global__ __launch_bounds__(TPB) void neg_mean_kernel(const float* __restrict__ q, int64_t b,
                                                       float g, float* __restrict__ grad,
                                                       double* __restrict__ partials,
                                                       float* __restrict__ loss) {
    __shared__ double red[NW];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * TPB + t;
    double term = 0.0;
    if (r < b) {
        term = (double)q[r];
        grad[r] = g;
    }
    const double ws = wave_sum(term);
    if ((t & (kWave - 1)) == 0) red[t / kWave] = ws;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < NW; ++i) s += red[i];
        if (gridDim.x == 1)
            finish_losses(&s, 1, b, -1.0f, loss, nullptr);
        else
            partials[blockIdx.x] = s;
    }
}

// partials [nk][nblk] -> loss[k] = sign * sum_blk / b, total (optional) = their sum.
__global__ void q_fold_kernel(const double* __restrict__ partials, int64_t nblk, int nk,
                              int64_t b, float sign, float* __restrict__ loss,
                              float* __restrict__ total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s[2] = {0.0, 0.0};
        for (int k = 0; k < nk; ++k)
            for (int64_t i = 0; i < nblk; ++i) s[k] += partials[(int64_t)k * nblk + i];
        finish_losses(s, nk, b, sign, loss, total);
    }
}

// NumPy's `act + noise` (f32 + f64 -> f64), rounded to the f32 the buffer and the critic use.
__global__ __launch_bounds__(TPB) void act_noise_kernel(const float* __restrict__ act,
                                                        const double* __restrict__ noise,
                                                        int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    out[i] = (float)((double)act[i] + noise[i]);
}

inline unsigned row_blocks(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }
inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_soft_update(float* t0, const float* s0, int64_t n0, float* t1,
                                const float* s1, int64_t n1, float* t2, const float* s2,
                                int64_t n2, float* t3, const float* s3, int64_t n3, double tau,
                                void* stream) {
    float* const ts[kMaxSeg] = {t0, t1, t2, t3};
    const float* const ss[kMaxSeg] = {s0, s1, s2, s3};
    const int64_t ns[kMaxSeg] = {n0, n1, n2, n3};
    TSRL_CHECK_ARG(tau >= 0.0 && tau <= 1.0, "tsrl_soft_update: tau must be in [0, 1]");
    Segs segs;
    int nseg = 0;
    int64_t longest = 0;
    for (int i = 0; i < kMaxSeg; ++i) {
        TSRL_CHECK_ARG(ns[i] >= 0, "tsrl_soft_update: segment %d has a negative length", i);
        if (ns[i] == 0) continue;
        TSRL_CHECK_ARG(ts[i] && ss[i], "tsrl_soft_update: segment %d has a null pointer", i);
        TSRL_CHECK_ARG(aligned4(ts[i]) && aligned4(ss[i]),
                       "tsrl_soft_update: segment %d is not 4-byte aligned", i);
        segs.seg[nseg++] = Seg{ts[i], ss[i], ns[i]};
        longest = ns[i] > longest ? ns[i] : longest;
    }
    if (nseg == 0) return 0;
    for (int i = nseg; i < kMaxSeg; ++i) segs.seg[i] = Seg{nullptr, nullptr, 0};
    const int64_t want = (longest / 4 + TPB - 1) / TPB + 1;
    const unsigned bx = (unsigned)(want < (int64_t)kMaxBlocks ? want : (int64_t)kMaxBlocks);
    hipLaunchKernelGGL(soft_update_kernel, dim3(bx, (unsigned)nseg), dim3(TPB), 0,
                       as_stream(stream), segs, (float)tau, (float)(1.0 - tau));
    TSRL_LAUNCH_CHECK("tsrl_soft_update");
    return 0;
}

extern "C" int tsrl_td3_smooth(const float* act, const float* noise, double sigma, double clip,
                               int64_t n, float* out, void* stream) {
    TSRL_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) * TPB, "tsrl_td3_smooth: need n >= 0");
    if (n == 0) return 0;
    TSRL_CHECK_ARG(act && noise && out, "tsrl_td3_smooth: null pointer");
    hipLaunchKernelGGL(td3_smooth_kernel, dim3(row_blocks(n)), dim3(TPB), 0, as_stream(stream),
                       act, noise, (float)sigma, (float)clip, n, out);
    TSRL_LAUNCH_CHECK("tsrl_td3_smooth");
    return 0;
}

extern "C" int64_t tsrl_ddpg_num_partials(int64_t b) { return b > 0 ? (b + TPB - 1) / TPB : 0; }

extern "C" int tsrl_q_mse_fwd_bwd(const float* q1, const float* q2, const float* returns,
                                  const float* weight, int64_t b, float* grad1, float* grad2,
                                  float* td_out, double* partials, float* loss, float* total,
                                  void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_q_mse_fwd_bwd: need b >= 1");
    TSRL_CHECK_ARG(q1 && returns && grad1 && td_out && loss && (!q2 || grad2),
                   "tsrl_q_mse_fwd_bwd: null pointer");
    const int64_t nblk = tsrl_ddpg_num_partials(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "tsrl_q_mse_fwd_bwd: b > %d needs partials", TPB);
    hipLaunchKernelGGL(q_mse_kernel, dim3((unsigned)nblk), dim3(TPB), 0, as_stream(stream), q1,
                       q2, returns, weight, b, 1.0f / (float)b, grad1, grad2, td_out, partials,
                       loss, total);
    TSRL_LAUNCH_CHECK("tsrl_q_mse_fwd_bwd");
    if (nblk > 1) {
        hipLaunchKernelGGL(q_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), partials,
                           nblk, q2 ? 2 : 1, b, 1.0f, loss, total);
        TSRL_LAUNCH_CHECK("tsrl_q_mse_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_neg_mean_fwd_bwd(const float* q, int64_t b, float* grad, double* partials,
                                     float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_neg_mean_fwd_bwd: need b >= 1");
    TSRL_CHECK_ARG(q && grad && loss, "tsrl_neg_mean_fwd_bwd: null pointer");
    const int64_t nblk = tsrl_ddpg_num_partials(b);
    TSRL_CHECK_ARG(nblk == 1 || partials, "tsrl_neg_mean_fwd_bwd: b > %d needs partials", TPB);
    hipLaunchKernelGGL(neg_mean_kernel, dim3((unsigned)nblk), dim3(TPB), 0, as_stream(stream), q,
                       b, -1.0f / (float)b, grad, partials, loss);
    TSRL_LAUNCH_CHECK("tsrl_neg_mean_fwd_bwd");
    if (nblk > 1) {
        hipLaunchKernelGGL(q_fold_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), partials,
                           nblk, 1, b, -1.0f, loss, (float*)nullptr);
        TSRL_LAUNCH_CHECK("tsrl_neg_mean_fwd_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_act_noise(const float* act, const double* noise, int64_t n, float* out,
                              void* stream) {
    TSRL_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31) * TPB, "tsrl_act_noise: need n >= 0");
    if (n == 0) return 0;
    TSRL_CHECK_ARG(act && noise && out, "tsrl_act_noise: null pointer");
    hipLaunchKernelGGL(act_noise_kernel, dim3(row_blocks(n)), dim3(TPB), 0, as_stream(stream),
                       act, noise, n, out);
    TSRL_LAUNCH_CHECK("tsrl_act_noise");
    return 0;
}
