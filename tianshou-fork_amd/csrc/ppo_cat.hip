// Fused PPO clipped-surrogate + value + entropy loss with its analytic gradient for
// Categorical policies (discrete actions; PPOPolicy.learn minibatch body,
// tianshou/policy/modelfree/ppo.py:106-151):
//   mode 0  Categorical(logits=x)  (examples/atari/atari_ppo.py:136-137, Actor with
//           softmax_output=False),
//   mode 1  Categorical(probs=x)   (test/discrete/test_ppo.py:95, Actor softmax output,
//           utils/net/discrete.py:69-70).
// torch's f32 formulation is followed step by step (torch/distributions/categorical.py,
// utils.py: logits = x - logsumexp(x); probs = softmax(logits) | probs = x / sum(x);
// logits = log(clamp(probs, eps, 1 - eps)); log_prob = logits[a]; entropy =
// -sum(clamp(logits, min=f32 min) * probs)), and its backward is written out: on ties min/max
// split the gradient in half and clamp passes it on the closed interval, as torch does.
// -inf logits (mode 0: masked, illegal actions) are in scope and follow torch: a masked entry
// has probability 0, contributes 0 to the entropy (the clamp at f32 min, in the forward and in
// the gradient alike) and gets gradient exactly 0; a row whose taken action is masked has
// log_prob -inf and ratio 0.  A row of all -inf is NaN (loss and gradient), as in torch.
// Accepted widths: 1 <= nA <= MAX_ACT = 64; the loss kernel stages 2 * 256 * nA floats of
// dynamic LDS per workgroup (2 KiB * nA: 128 KiB at nA = 64).  Wider inputs are an argument
// error; the Python layer takes the torch path for them (policy/fused_mlp.py LOSS_MAX_ACT).
// One workgroup = 256 minibatch rows; the [256, nA] tile of x (contiguous, minibatch order)
// is staged in LDS, the gathered rows of act/logp_old/adv/returns/v_s come through idx.
#include "ppo_loss.h"

namespace tsrl {
namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / kWave;
constexpr int MAX_ACT = 64;
constexpr float F32_EPS = 1.1920928955078125e-07f;
constexpr float F32_MIN = -3.4028234663852886e+38f;

// Row quantities of the distribution: normalised logits l[] and probabilities q[] (in place
// over the LDS row), the sum S (probs mode), returns entropy.  clamp masks in m (probs mode).
struct Row {
    float H;
    float S;
};

__device__ __forceinline__ Row cat_row(float* x, float* l, int A, int mode, uint64_t* mask) {
    Row o;
    o.S = 1.0f;
    *mask = 0;
    if (mode == 0) {
        float mx = -INFINITY;
        for (int j = 0; j < A; ++j) mx = fmaxf(mx, x[j]);
        float se = 0.0f;
        for (int j = 0; j < A; ++j) se += expf(x[j] - mx);
        const float lse = mx + logf(se);
        float m2 = -INFINITY;
        for (int j = 0; j < A; ++j) {
            l[j] = x[j] - lse;
            m2 = fmaxf(m2, l[j]);
        }
        float s2 = 0.0f;
        for (int j = 0; j < A; ++j) {
            const float e = expf(l[j] - m2);
            x[j] = e;  // x now holds probs
            s2 += e;
        }
        for (int j = 0; j < A; ++j) x[j] = x[j] / s2;
    } else {
        float S = 0.0f;
        for (int j = 0; j < A; ++j) S += x[j];
        o.S = S;
        for (int j = 0; j < A; ++j) {
            const float q = x[j] / S;
            x[j] = q;
            const float qc = fminf(fmaxf(q, F32_EPS), 1.0f - F32_EPS);
            if (q >= F32_EPS && q <= 1.0f - F32_EPS) *mask |= 1ull << j;
            l[j] = logf(qc);
        }
    }
    // the f32 products summed in f64 and rounded once (a single row of 32 actions showed an
    // f32 running sum 2.7 ulp off, where torch's sum(-1) is within one)
    double h = 0.0;
    for (int j = 0; j < A; ++j) h += (double)(fmaxf(l[j], F32_MIN) * x[j]);
    o.H = (float)(-h);
    return o;
}

__global__ __launch_bounds__(TPB) void cat_fwd_bwd_kernel(
    const float* xin, const float* value, const int64_t* act, const float* logp_old,
    const float* adv, const float* ret, const float* v_s, const int64_t* idx, int64_t b,
    int A, int mode, const double* adv_sums, LossParams p, float* grad_x, float* grad_value,
    double* partials) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_x = smem;             // [TPB * A]  x -> probs -> grad
    float* s_l = smem + TPB * A;   // [TPB * A]  normalised logits
    __shared__ double red[NW][4];
    const int w = threadIdx.x / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t r0 = (int64_t)blockIdx.x * TPB;
    const int nrows = (int)min((int64_t)TPB, b - r0);
    const int nel = nrows * A;
    const float* x_blk = xin + r0 * A;
    for (int f = threadIdx.x; f < nel; f += TPB) s_x[f] = x_blk[f];
    __syncthreads();
    float mean_f = 0.0f, std_f = 1.0f;
    if (p.norm_adv) adv_mean_std(adv_sums, p.inv_b, mean_f, std_f);
    const int t = threadIdx.x;
    const bool live = t < nrows;
    double clip_term = 0.0, vf_term = 0.0, ent_term = 0.0;
    if (live) {
        const int64_t r = r0 + t;
        const int64_t j = idx ? idx[r] : r;
        float* q = s_x + t * A;
        float* l = s_l + t * A;
        uint64_t mask;
        const Row row = cat_row(q, l, A, mode, &mask);
        const int64_t a64 = act[j];
        const int a = (a64 >= 0 && a64 < A) ? (int)a64 : -1;  // invalid action -> NaN loss
        const float logp = a >= 0 ? l[a] : NAN;
        float an = adv[j];
        if (p.norm_adv) an = (an - mean_f) / (std_f + p.adv_eps);
        const PolicyTerm pt =
            policy_term(logp, p.objective == OBJ_A2C ? 0.0f : logp_old[j], an, p);
        clip_term = -(double)pt.obj;
        ent_term = (double)row.H;
        const float c_lp = (float)(-pt.dlogp * p.inv_b);
        const float c_h = (float)(-(double)p.ent_coef * p.inv_b);
        // d(loss)/dx in place over the probs row
        if (mode == 0) {
            for (int k = 0; k < A; ++k) {
                const float qk = q[k];
                // the clamped logit, as in the entropy above: a masked entry (l = -inf, q = 0)
                // gets gradient 0, not 0 * inf
                const float g = c_lp * ((k == a ? 1.0f : 0.0f) - qk) +
                                c_h * (-qk * (fmaxf(l[k], F32_MIN) + row.H));
                l[k] = g;
            }
            for (int k = 0; k < A; ++k) q[k] = l[k];
        } else {
            float dot = 0.0f;
            for (int k = 0; k < A; ++k) {
                const float qk = q[k];
                const float dl = (k == a ? c_lp : 0.0f) - c_h * qk;
                const float g = ((mask >> k) & 1ull ? dl / qk : 0.0f) - c_h * l[k];
                l[k] = g;
                dot += g * qk;
            }
            for (int k = 0; k < A; ++k) q[k] = (l[k] - dot) / row.S;
        }
        const ValueLoss vl = value_loss(value[r], ret[j], p.value_clip ? v_s[j] : 0.0f, p);
        vf_term = (double)vl.vf;
        grad_value[r] = (float)((double)p.vf_coef * (double)vl.dv * p.inv_b);
    }
    const double cs = wave_sum(clip_term);
    const double vs = wave_sum(vf_term);
    const double cnt = wave_sum(live ? 1.0 : 0.0);
    const double es = wave_sum(ent_term);
    if (lane == 0) {
        red[w][0] = cs;
        red[w][1] = vs;
        red[w][2] = cnt;
        red[w][3] = es;
    }
    __syncthreads();
    float* g_blk = grad_x + r0 * A;
    for (int f = threadIdx.x; f < nel; f += TPB) g_blk[f] = s_x[f];
    // as gauss_fwd_bwd_kernel's epilogue (same wave order), with 4 columns
    if (threadIdx.x < 4) {
        double tsum = 0.0;
        for (int i = 0; i < NW; ++i) tsum += red[i][threadIdx.x];
        partials[(int64_t)blockIdx.x * 4 + threadIdx.x] = tsum;
    }
}

// not ppo_loss.h's gauss_finalize: the entropy here is a reduced sum (sums[3])
__global__ void cat_finalize_kernel(const double* sums, LossParams p, float* losses) {
    if (threadIdx.x == 0) {
        const float clip = (float)(sums[0] * p.inv_b);
        const float vf = (float)(sums[1] * p.inv_b);
        const float ent = (float)(sums[3] * p.inv_b);
        losses[0] = clip + p.vf_coef * vf - p.ent_coef * ent;
        losses[1] = clip;
        losses[2] = vf;
        losses[3] = ent;
    }
}

__global__ __launch_bounds__(TPB) void cat_logp_kernel(const float* xin, const int64_t* act,
                                                       int64_t b, int A, int mode, float* out) {
    float l[MAX_ACT], q[MAX_ACT];
    for (int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x; r < b;
         r += (int64_t)gridDim.x * TPB) {
        for (int j = 0; j < A; ++j) q[j] = xin[r * A + j];
        uint64_t mask;
        cat_row(q, l, A, mode, &mask);
        const int64_t a = act[r];
        out[r] = (a >= 0 && a < A) ? l[(int)a] : NAN;
    }
}

// Categorical(logits).sample() as one pass (Collector step, pg.py:133-171 -> dist.sample()):
// the Gumbel-max form argmax_a(logits[a] - log(-log(u[a]))) with u ~ U[0, 1) drawn by the
// caller (torch.rand_like: torch's own, graph-capturable stream), which samples exactly the
// categorical distribution of the logits (first index on ties; -inf logits are never drawn).
// Replaces torch's softmax + multinomial (exponential draw, argmax and its validity
// reductions): ~14 small kernels per collector step for Atari-sized batches.
__global__ __launch_bounds__(TPB) void cat_gumbel_argmax_kernel(const float* __restrict__ logits,
                                                                const float* __restrict__ u,
                                                                int64_t n, int64_t A,
                                                                int64_t* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= n) return;
    const float* lr = logits + r * A;
    const float* ur = u + r * A;
    float best = -INFINITY;
    int64_t arg = 0;
    for (int64_t a = 0; a < A; ++a) {
        const float g = lr[a] - logf(-logf(ur[a]));
        if (g > best) {
            best = g;
            arg = a;
        }
    }
    out[r] = arg;
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_ppo_cat_fwd_bwd(const float* x, const float* value, const int64_t* act,
                                    const float* logp_old, const float* adv, const float* ret,
                                    const float* v_s, const int64_t* idx, int64_t b,
                                    int64_t num_actions, int mode, const double* adv_sums,
                                    tsrl_ppo_params p, float* grad_x, float* grad_value,
                                    double* partials, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && num_actions > 0 && num_actions <= MAX_ACT,
                   "tsrl_ppo_cat_fwd_bwd: need 0 < num_actions <= %d", MAX_ACT);
    TSRL_CHECK_ARG(mode == 0 || mode == 1, "tsrl_ppo_cat_fwd_bwd: mode must be 0 or 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(x && value && act && adv && ret && grad_x && grad_value && partials,
                   "tsrl_ppo_cat_fwd_bwd: null pointer");
    TSRL_CHECK_ARG(objective_args_ok(p, logp_old),
                   "tsrl_ppo_cat_fwd_bwd: objective 0 needs logp_old; objective 1 takes no "
                   "norm_adv, value_clip or dual_clip");
    TSRL_CHECK_ARG(!p.value_clip || v_s, "tsrl_ppo_cat_fwd_bwd: value_clip needs v_s");
    TSRL_CHECK_ARG(!p.norm_adv || adv_sums, "tsrl_ppo_cat_fwd_bwd: norm_adv needs adv_sums");
    TSRL_CHECK_ARG(p.b_global >= 1.0, "tsrl_ppo_cat_fwd_bwd: b_global < 1");
    const size_t lds = 2 * (size_t)TPB * (size_t)num_actions * sizeof(float);
    hipLaunchKernelGGL(cat_fwd_bwd_kernel, dim3((unsigned)((b + TPB - 1) / TPB)), dim3(TPB), lds,
                       as_stream(stream), x, value, act, logp_old, adv, ret, v_s, idx, b,
                       (int)num_actions, mode, adv_sums, make_loss_params(p), grad_x, grad_value,
                       partials);
    TSRL_LAUNCH_CHECK("tsrl_ppo_cat_fwd_bwd");
    return 0;
}

extern "C" int tsrl_ppo_cat_finalize(const double* sums, tsrl_ppo_params p, float* losses,
                                     void* stream) {
    TSRL_CHECK_ARG(sums && losses, "tsrl_ppo_cat_finalize: null pointer");
    hipLaunchKernelGGL(cat_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), sums,
                       make_loss_params(p), losses);
    TSRL_LAUNCH_CHECK("tsrl_ppo_cat_finalize");
    return 0;
}

extern "C" int tsrl_cat_logp(const float* x, const int64_t* act, int64_t b, int64_t num_actions,
                             int mode, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && num_actions > 0 && num_actions <= MAX_ACT,
                   "tsrl_cat_logp: need 0 < num_actions <= %d", MAX_ACT);
    TSRL_CHECK_ARG(mode == 0 || mode == 1, "tsrl_cat_logp: mode must be 0 or 1");
    if (b == 0) return 0;
    TSRL_CHECK_ARG(x && act && out, "tsrl_cat_logp: null pointer");
    const int64_t grid = std::min<int64_t>((b + TPB - 1) / TPB, 16384);
    hipLaunchKernelGGL(cat_logp_kernel, dim3((unsigned)grid), dim3(TPB), 0, as_stream(stream), x,
                       act, b, (int)num_actions, mode, out);
    TSRL_LAUNCH_CHECK("tsrl_cat_logp");
    return 0;
}

extern "C" int tsrl_cat_gumbel_argmax(const float* logits, const float* u, int64_t n,
                                      int64_t num_actions, int64_t* out, void* stream) {
    TSRL_CHECK_ARG(n >= 0 && num_actions > 0, "tsrl_cat_gumbel_argmax: bad sizes");
    if (n == 0) return 0;
    TSRL_CHECK_ARG(logits && u && out, "tsrl_cat_gumbel_argmax: null pointer");
    hipLaunchKernelGGL(cat_gumbel_argmax_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB),
                       0, as_stream(stream), logits, u, n, num_actions, out);
    TSRL_LAUNCH_CHECK("tsrl_cat_gumbel_argmax");
    return 0;
}
