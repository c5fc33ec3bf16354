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
#include "loss_sum.h"

namespace tsrl {
namespace {

constexpr int TPB = kLossTPB;
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

// One workgroup = 256 rows of the NK critics (q2 and grad2 are read only with NK = 2).  The loss
// terms are summed in loss_sum.h's fixed order.
template <int NK>
__global__ __launch_bounds__(TPB) void q_mse_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ returns, const float* __restrict__ weight, int64_t b, float inv_b,
    float* __restrict__ grad1, float* __restrict__ grad2, float* __restrict__ td_out,
    double* __restrict__ partials, MeanLosses<NK> fin) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[NK] = {};
    if (r < b) {
        const float ret = returns[r];
        const float w = weight ? weight[r] : 1.0f;
        const float td1 = q1[r] - ret;
        term[0] = (double)(td1 * td1 * w);
        grad1[r] = 2.0f * td1 * w * inv_b;
        float row = td1;
        if constexpr (NK == 2) {
            const float td2 = q2[r] - ret;
            term[1] = (double)(td2 * td2 * w);
            grad2[r] = 2.0f * td2 * w * inv_b;
            row = (td1 + td2) / 2.0f;
        }
        td_out[r] = row;
    }
    double s[NK];
    block_sums<NK>(term, s);
    losses_or_partials<NK>(s, partials, fin);
}

__global__ __launch_bounds__(TPB) void neg_mean_kernel(const float* __restrict__ q, int64_t b,
                                                       float g, float* __restrict__ grad,
                                                       double* __restrict__ partials,
                                                       MeanLosses<1> fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[1] = {0.0};
    if (r < b) {
        term[0] = (double)q[r];
        grad[r] = g;
    }
    double s[1];
    block_sums<1>(term, s);
    losses_or_partials<1>(s, partials, fin);
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

template <int NK>
int launch_q_mse(const float* q1, const float* q2, const float* returns, const float* weight,
                 int64_t b, float* grad1, float* grad2, float* td_out, double* partials,
                 float* loss, float* total, hipStream_t st) {
    const MeanLosses<NK> fin{(double)b, 1.0f, loss, total};
    return launch_loss<NK>("tsrl_q_mse_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(q_mse_kernel<NK>, dim3(nblk), dim3(TPB), 0, st, q1, q2, returns,
                           weight, b, 1.0f / (float)b, grad1, grad2, td_out, partials, fin);
    });
}

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

extern "C" int64_t tsrl_ddpg_num_partials(int64_t b) { return loss_blocks(b); }

extern "C" int tsrl_q_mse_fwd_bwd(const float* q1, const float* q2, const float* returns,
                                  const float* weight, int64_t b, float* grad1, float* grad2,
                                  float* td_out, double* partials, float* loss, float* total,
                                  void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_q_mse_fwd_bwd: need b >= 1");
    TSRL_CHECK_ARG(q1 && returns && grad1 && td_out && loss && (!q2 || grad2),
                   "tsrl_q_mse_fwd_bwd: null pointer");
    return (q2 ? launch_q_mse<2> : launch_q_mse<1>)(q1, q2, returns, weight, b, grad1, grad2,
                                                    td_out, partials, loss, total,
                                                    as_stream(stream));
}

extern "C" int tsrl_neg_mean_fwd_bwd(const float* q, int64_t b, float* grad, double* partials,
                                     float* loss, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && b < ((int64_t)1 << 31) * TPB, "tsrl_neg_mean_fwd_bwd: need b >= 1");
    TSRL_CHECK_ARG(q && grad && loss, "tsrl_neg_mean_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const MeanLosses<1> fin{(double)b, -1.0f, loss, nullptr};
    return launch_loss<1>("tsrl_neg_mean_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(neg_mean_kernel, dim3(nblk), dim3(TPB), 0, st, q, b,
                           -1.0f / (float)b, grad, partials, fin);
    });
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
