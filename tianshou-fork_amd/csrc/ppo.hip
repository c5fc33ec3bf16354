// Fused PPO clipped-surrogate + value + entropy loss with its analytic gradient
// (PPOPolicy.learn minibatch body, tianshou/policy/modelfree/ppo.py:106-151) for the
// Gaussian actor Independent(Normal(mu, exp(log_std)), 1) with state-independent log_std
// (ActorProb, utils/net/continuous.py:218-235; fixed_std_normal, utils/models.py:96-97).
//
// One pass over the minibatch rows: gathers act/logp_old/adv/returns/v_s through the
// minibatch index (no materialised minibatch copy), computes log-prob, ratio, the clipped
// objective (dual-clip optional), the value loss (value-clip optional), and writes
// d(mean loss)/d(mu) [b, A] and d/d(value) [b] directly; per-block partial sums of the loss
// terms and of d/d(log_std) are reduced deterministically (fixed order) afterwards.
// torch's tie rules are reproduced: min/max split the gradient in half on ties, clamp passes
// it on the closed interval.
#include "ppo_loss.h"

namespace tsrl {
namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / kWave;
constexpr int MAX_ACT = 64;

// Block sums of a per-thread (s, ss) pair: wave sums, then threads 0 and 1 add the waves in
// order and write out[0] = sum of s, out[1] = sum of ss.
__device__ __forceinline__ void block_sum2(double s, double ss, double* out) {
    __shared__ double sh[NW][2];
    s = wave_sum(s);
    ss = wave_sum(ss);
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sh[w][0] = s;
        sh[w][1] = ss;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
        for (int i = 0; i < NW; ++i) t += sh[i][threadIdx.x];
        out[threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(TPB) void adv_moments_kernel(const float* adv, const int64_t* idx,
                                                          int64_t b, double* partials) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double s = 0.0, ss = 0.0;
    if (r < b) {
        const double a = (double)adv[idx ? idx[r] : r];
        s = a;
        ss = a * a;
    }
    block_sum2(s, ss, partials + 2 * blockIdx.x);
}

__global__ __launch_bounds__(TPB) void reduce_partials_kernel(const double* partials,
                                                              int64_t nblk, int64_t width,
                                                              double* out) {
    __shared__ double sh[TPB];
    for (int64_t c = 0; c < width; ++c) {
        double s = 0.0;
        for (int64_t i = threadIdx.x; i < nblk; i += TPB) s += partials[i * width + c];
        sh[threadIdx.x] = s;
        __syncthreads();
        for (int st = TPB / 2; st > 0; st >>= 1) {
            if (threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[c] = sh[0];
        __syncthreads();
    }
}

// Advantage moments of every minibatch of an epoch at once (one all-reduce per epoch under
// data parallelism instead of one per minibatch).  Segment g = rows [bounds[g], bounds[g+1])
// of idx; workgroup (p, g) folds a strided 1/nparts share of segment g into partials[g][p],
// then one workgroup per segment sums its partials in fixed order.
__global__ __launch_bounds__(TPB) void adv_moments_seg_kernel(const float* adv, const int64_t* idx,
                                                              const int64_t* bounds, int nparts,
                                                              double* partials) {
    const int g = blockIdx.y;
    const int64_t s0 = bounds[g], s1 = bounds[g + 1];
    double s = 0.0, ss = 0.0;
    for (int64_t r = s0 + (int64_t)blockIdx.x * TPB + threadIdx.x; r < s1;
         r += (int64_t)nparts * TPB) {
        const double a = (double)adv[idx ? idx[r] : r];
        s += a;
        ss += a * a;
    }
    block_sum2(s, ss, partials + ((int64_t)g * nparts + blockIdx.x) * 2);
}

__global__ __launch_bounds__(kWave) void adv_moments_seg_reduce_kernel(const double* partials,
                                                                       int nparts, double* out) {
    const int g = blockIdx.x;
    double s = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kWave) {
        s += partials[((int64_t)g * nparts + i) * 2];
        ss += partials[((int64_t)g * nparts + i) * 2 + 1];
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (threadIdx.x == 0) {
        out[2 * g] = s;
        out[2 * g + 1] = ss;
    }
}

// One workgroup = 256 minibatch rows.  The [256, A] mu tile (contiguous) and the gathered
// act rows are staged through LDS with coalesced / row-contiguous loads, the per-row math
// reads LDS (row stride A: conflict-free for odd A), and grad_mu goes back out through the
// same LDS tile as one contiguous coalesced store.
__global__ __launch_bounds__(TPB) void gauss_fwd_bwd_kernel(
    const float* mu, const float* log_std, const float* value, const float* act,
    const float* logp_old, const float* adv, const float* ret, const float* v_s,
    const int64_t* idx, int64_t b, int64_t A, const double* adv_sums, LossParams p,
    float* grad_mu, float* grad_value, double* partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_mu = smem;             // [TPB * A]
    float* s_act = smem + TPB * A;  // [TPB * A]
    __shared__ float s_var[MAX_ACT], s_ls[MAX_ACT];
    __shared__ double red[NW][4 + MAX_ACT];
    const int w = threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r0 = (int64_t)blockIdx.x * TPB;
    const int nrows = (int)min((int64_t)TPB, b - r0);
    for (int a = threadIdx.x; a < A; a += TPB) {
        const float sig = expf(log_std[a]);
        s_var[a] = sig * sig;
        s_ls[a] = logf(sig);
    }
    const int nel = nrows * (int)A;
    const float* mu_blk = mu + r0 * A;
    for (int f = threadIdx.x; f < nel; f += TPB) s_mu[f] = mu_blk[f];
    for (int f = threadIdx.x; f < nel; f += TPB) {
        const int row = f / (int)A;
        const int a = f - row * (int)A;
        const int64_t j = idx ? idx[r0 + row] : r0 + row;
        s_act[f] = act[j * A + a];
    }
    __syncthreads();
    float mean_f = 0.0f, std_f = 1.0f;
    if (p.norm_adv) adv_mean_std(adv_sums, p.inv_b, mean_f, std_f);
    const int t = threadIdx.x;
    const bool live = t < nrows;
    const int64_t r = r0 + t;
    const int64_t j = live ? (idx ? idx[r] : r) : 0;
    float* my_mu = s_mu + t * A;
    const float* my_act = s_act + t * A;
    float g_logp = 0.0f;
    double clip_term = 0.0, vf_term = 0.0;
    if (live) {
        float an = adv[j];
        if (p.norm_adv) an = (an - mean_f) / (std_f + p.adv_eps);
        // the f32 terms summed in f64 and rounded once: an f32 running sum over 64 terms loses
        // ~5x the accuracy of torch's sum(-1), which the ratio exp(logp - logp_old) then shows
        double lp = 0.0;
        for (int64_t a = 0; a < A; ++a) {
            const float diff = my_act[a] - my_mu[a];
            lp += (double)gauss_logp_term(diff, s_var[a], s_ls[a]);
        }
        const float logp = (float)lp;
        const PolicyTerm pt =
            policy_term(logp, p.objective == OBJ_A2C ? 0.0f : logp_old[j], an, p);
        clip_term = -(double)pt.obj;
        g_logp = (float)(-pt.dlogp * p.inv_b);

        const ValueLoss vl = value_loss(value[r], ret[j], p.value_clip ? v_s[j] : 0.0f, p);
        vf_term = (double)vl.vf;
        grad_value[r] = (float)((double)p.vf_coef * (double)vl.dv * p.inv_b);
    }
    // d/d(mu) into the LDS tile (own row only), d/d(log_std) partials per dim
    for (int64_t a = 0; a < A; ++a) {
        double dls = 0.0;
        if (live) {
            const float diff = my_act[a] - my_mu[a];
            const float var = s_var[a];
            my_mu[a] = g_logp * diff / var;
            dls = (double)g_logp * ((double)(diff * diff) / (double)var - 1.0);
        }
        dls = wave_sum(dls);
        if (lane == 0) red[w][4 + a] = dls;
    }
    const double cs = wave_sum(clip_term);
    const double vs = wave_sum(vf_term);
    const double cnt = wave_sum(live ? 1.0 : 0.0);
    if (lane == 0) {
        red[w][0] = cs;
        red[w][1] = vs;
        red[w][2] = cnt;
        red[w][3] = 0.0;
    }
    __syncthreads();
    float* gm_blk = grad_mu + r0 * A;
    for (int f = threadIdx.x; f < nel; f += TPB) gm_blk[f] = s_mu[f];
    // not block_sum2: 4 + A columns per wave, one thread per column
    for (int c = threadIdx.x; c < 4 + A; c += TPB) {
        double tsum = 0.0;
        for (int i = 0; i < NW; ++i) tsum += red[i][c];
        partials[(int64_t)blockIdx.x * (4 + A) + c] = tsum;
    }
}

__global__ void gauss_finalize_kernel(const double* sums, int A, const float* log_std,
                                      LossParams p, float* losses, float* grad_log_std) {
    gauss_finalize<double>(sums, A, log_std, p.vf_coef, p.ent_coef, p.inv_b, losses,
                           grad_log_std);
}

__global__ __launch_bounds__(TPB) void gauss_logp_kernel(const float* mu, const float* log_std,
                                                         const float* act, int64_t b, int64_t A,
                                                         float* out) {
    __shared__ float s_var[MAX_ACT], s_ls[MAX_ACT];
    for (int a = threadIdx.x; a < A; a += TPB) {
        const float sig = expf(log_std[a]);
        s_var[a] = sig * sig;
        s_ls[a] = logf(sig);
    }
    __syncthreads();
    for (int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x; r < b;
         r += (int64_t)gridDim.x * TPB) {
        double lp = 0.0;  // as gauss_fwd_bwd_kernel: the same bits, so an unchanged policy has ratio 1
        for (int64_t a = 0; a < A; ++a) {
            const float diff = act[r * A + a] - mu[r * A + a];
            lp += (double)gauss_logp_term(diff, s_var[a], s_ls[a]);
        }
        out[r] = (float)lp;
    }
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int64_t tsrl_ppo_num_partials(int64_t b) { return (b + TPB - 1) / TPB; }

extern "C" int tsrl_adv_moments(const float* adv, const int64_t* idx, int64_t b,
                                double* partials, void* stream) {
    TSRL_CHECK_ARG(b >= 0, "tsrl_adv_moments: b < 0");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(adv && partials, "tsrl_adv_moments: null pointer");
    hipLaunchKernelGGL(adv_moments_kernel, dim3((unsigned)tsrl_ppo_num_partials(b)), dim3(TPB), 0,
                       as_stream(stream), adv, idx, b, partials);
    TSRL_LAUNCH_CHECK("tsrl_adv_moments");
    return 0;
}

extern "C" int64_t tsrl_adv_moments_seg_parts(int64_t max_seg) {
    const int64_t p = (max_seg + 4 * TPB - 1) / (4 * TPB);  // ~4 rows per thread
    return p < 1 ? 1 : (p > 256 ? 256 : p);
}

extern "C" int tsrl_adv_moments_seg(const float* adv, const int64_t* idx, const int64_t* bounds,
                                    int64_t nseg, int64_t max_seg, double* partials,
                                    double* out, void* stream) {
    TSRL_CHECK_ARG(nseg >= 0 && nseg <= 65535 && max_seg >= 0,
                   "tsrl_adv_moments_seg: nseg=%lld max_seg=%lld", (long long)nseg,
                   (long long)max_seg);
    if (nseg == 0) return 0;
    TSRL_CHECK_ARG(adv && bounds && partials && out, "tsrl_adv_moments_seg: null pointer");
    const int nparts = (int)tsrl_adv_moments_seg_parts(max_seg);
    hipLaunchKernelGGL(adv_moments_seg_kernel, dim3((unsigned)nparts, (unsigned)nseg), dim3(TPB),
                       0, as_stream(stream), adv, idx, bounds, nparts, partials);
    TSRL_LAUNCH_CHECK("adv_moments_seg_kernel");
    hipLaunchKernelGGL(adv_moments_seg_reduce_kernel, dim3((unsigned)nseg), dim3(kWave), 0,
                       as_stream(stream), partials, nparts, out);
    TSRL_LAUNCH_CHECK("adv_moments_seg_reduce_kernel");
    return 0;
}

extern "C" int tsrl_reduce_partials(const double* partials, int64_t nblk, int64_t width,
                                    double* out, void* stream) {
    TSRL_CHECK_ARG(partials && out && nblk >= 0 && width > 0, "tsrl_reduce_partials: bad args");
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(TPB), 0, as_stream(stream), partials,
                       nblk, width, out);
    TSRL_LAUNCH_CHECK("tsrl_reduce_partials");
    return 0;
}

extern "C" int tsrl_ppo_gauss_fwd_bwd(const float* mu, const float* log_std, const float* value,
                                      const float* act, const float* logp_old, const float* adv,
                                      const float* ret, const float* v_s, const int64_t* idx,
                                      int64_t b, int64_t act_dim, const double* adv_sums,
                                      tsrl_ppo_params p, float* grad_mu, float* grad_value,
                                      double* partials, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && act_dim > 0 && act_dim <= MAX_ACT,
                   "tsrl_ppo_gauss_fwd_bwd: need 0 < act_dim <= %d", MAX_ACT);
    if (b == 0) return 0;
    TSRL_CHECK_ARG(mu && log_std && value && act && adv && ret && grad_mu && grad_value &&
                       partials,
                   "tsrl_ppo_gauss_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(objective_args_ok(p, logp_old),
                   "tsrl_ppo_gauss_fwd_bwd: objective 0 needs logp_old; objective 1 takes no "
                   "norm_adv, value_clip or dual_clip");
    TSRL_CHECK_ARG(!p.value_clip || v_s, "tsrl_ppo_gauss_fwd_bwd: value_clip needs v_s");
    TSRL_CHECK_ARG(!p.norm_adv || adv_sums, "tsrl_ppo_gauss_fwd_bwd: norm_adv needs adv_sums");
    TSRL_CHECK_ARG(p.b_global >= 1.0, "tsrl_ppo_gauss_fwd_bwd: b_global < 1");
    const size_t lds = 2 * (size_t)TPB * (size_t)act_dim * sizeof(float);
    hipLaunchKernelGGL(gauss_fwd_bwd_kernel, dim3((unsigned)tsrl_ppo_num_partials(b)), dim3(TPB),
                       lds, as_stream(stream), mu, log_std, value, act, logp_old, adv, ret, v_s,
                       idx, b, act_dim, adv_sums, make_loss_params(p), grad_mu, grad_value,
                       partials);
    TSRL_LAUNCH_CHECK("tsrl_ppo_gauss_fwd_bwd");
    return 0;
}

extern "C" int tsrl_ppo_gauss_finalize(const double* sums, int64_t act_dim, const float* log_std,
                                       tsrl_ppo_params p, float* losses, float* grad_log_std,
                                       void* stream) {
    TSRL_CHECK_ARG(sums && log_std && losses && grad_log_std && act_dim > 0 &&
                       act_dim <= MAX_ACT,
                   "tsrl_ppo_gauss_finalize: bad arguments");
    hipLaunchKernelGGL(gauss_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), sums,
                       (int)act_dim, log_std, make_loss_params(p), losses, grad_log_std);
    TSRL_LAUNCH_CHECK("tsrl_ppo_gauss_finalize");
    return 0;
}

extern "C" int tsrl_gauss_logp(const float* mu, const float* log_std, const float* act,
                               int64_t b, int64_t act_dim, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && act_dim > 0 && act_dim <= MAX_ACT, "tsrl_gauss_logp: bad sizes");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(mu && log_std && act && out, "tsrl_gauss_logp: null pointer");
    const int64_t grid = std::min<int64_t>((b + TPB - 1) / TPB, 16384);
    hipLaunchKernelGGL(gauss_logp_kernel, dim3((unsigned)grid), dim3(TPB), 0, as_stream(stream),
                       mu, log_std, act, b, act_dim, out);
    TSRL_LAUNCH_CHECK("tsrl_gauss_logp");
    return 0;
}
