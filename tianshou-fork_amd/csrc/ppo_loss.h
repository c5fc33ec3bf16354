// The per-row PPO minibatch loss (PPOPolicy.learn, tianshou/policy/modelfree/ppo.py:106-151),
// defined once for the kernels that compute it: gauss_fwd_bwd_kernel (ppo.hip),
// cat_fwd_bwd_kernel (ppo_cat.hip) and ppo_tail16_kernel (mlp.hip).  The clipped surrogate
// with optional dual clip, the value loss with optional value clip, and their analytic
// gradients; and, as objective 1, A2CPolicy.learn's policy term -(log_prob * adv)
// (a2c.py:126-137), which shares everything but policy_term.  torch's tie rules are
// reproduced: min/max split the gradient in half on ties, clamp passes it on the closed
// interval.  The order of operations and every float/double cast here are part of the
// numerical contract (tests/test_gpu_update_full.py, the goldens).
#pragma once
#include "tsrl_common.h"

namespace tsrl {

constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;  // math.log(math.sqrt(2*pi))

struct LossParams {
    float lo, hi, eps_clip, dual, vf_coef, ent_coef, adv_eps;
    int value_clip, norm_adv, use_dual;
    int objective;  // OBJ_PPO or OBJ_A2C
    double inv_b;
};

constexpr int OBJ_PPO = 0, OBJ_A2C = 1;

// The A2C objective (A2CPolicy.learn, a2c.py:126-137) has no clip, no advantage normalisation
// and no second value term: NULL logp_old / v_s are fine, those three options are not.
inline bool objective_args_ok(const tsrl_ppo_params& p, const void* logp_old) {
    if (p.objective == OBJ_PPO) return logp_old != nullptr;
    return p.objective == OBJ_A2C && !p.norm_adv && !p.value_clip && !(p.dual_clip > 0.0);
}

inline LossParams make_loss_params(const tsrl_ppo_params& p) {
    LossParams q;
    q.lo = (float)(1.0 - p.eps_clip);
    q.hi = (float)(1.0 + p.eps_clip);
    q.eps_clip = (float)p.eps_clip;
    q.dual = (float)p.dual_clip;
    q.use_dual = p.dual_clip > 0.0;
    q.vf_coef = (float)p.vf_coef;
    q.ent_coef = (float)p.ent_coef;
    q.adv_eps = (float)p.adv_eps;
    q.value_clip = p.value_clip;
    q.norm_adv = p.norm_adv;
    q.objective = p.objective;
    q.inv_b = 1.0 / p.b_global;
    return q;
}

// One action dimension's term of log N(act | mu, sigma): diff = act - mu, var = sigma^2,
// ls = log sigma.  (ppo_tail16_kernel multiplies by a precomputed 1 / (2 var) instead, which
// rounds differently, and keeps its own expression.)
__device__ __forceinline__ float gauss_logp_term(float diff, float var, float ls) {
    return -(diff * diff) / (2.0f * var) - ls - LOG_SQRT_2PI;
}

// Mean and unbiased std of the minibatch advantages from adv_sums = (sum, sum of squares)
// over n = 1 / inv_b rows.
__device__ __forceinline__ void adv_mean_std(const double* adv_sums, double inv_b, float& mean,
                                             float& std) {
    const double n = 1.0 / inv_b;
    const double m = adv_sums[0] / n;
    const double var = (adv_sums[1] - adv_sums[0] * m) / (n - 1.0);
    mean = (float)m;
    std = (float)sqrt(var > 0.0 ? var : 0.0);
}

// obj = min(ratio an, clamp(ratio, lo, hi) an), under dual clip max(obj, dual an) where
// an < 0; dobj = d(obj)/d(ratio).
struct Surrogate {
    float obj, dobj;
};

__device__ __forceinline__ Surrogate surrogate(float ratio, float an, const LossParams& p) {
    const float surr1 = ratio * an;
    const float rc = fminf(fmaxf(ratio, p.lo), p.hi);
    const float surr2 = rc * an;
    const float in_rng = (ratio >= p.lo && ratio <= p.hi) ? 1.0f : 0.0f;
    float clip1, d1;
    if (surr1 < surr2) {
        clip1 = surr1;
        d1 = an;
    } else if (surr2 < surr1) {
        clip1 = surr2;
        d1 = in_rng * an;
    } else {
        clip1 = surr1;
        d1 = 0.5f * an + 0.5f * in_rng * an;
    }
    float obj = clip1, dobj = d1;
    if (p.use_dual && an < 0.0f) {
        const float tt = p.dual * an;
        if (clip1 > tt) {
            obj = clip1;
        } else if (clip1 < tt) {
            obj = tt;
            dobj = 0.0f;
        } else {
            obj = clip1;
            dobj = 0.5f * d1;
        }
    }
    return {obj, dobj};
}

// The policy term of one row: obj, the objective the loss negates, and dlogp = d(obj)/d(logp)
// in f64 (the callers scale it by -1 / b in f64 and round once).  an is the (normalised)
// advantage.
//   PPO: ratio = exp(logp - logp_old), obj = surrogate(ratio), dlogp = dobj * ratio;
//   A2C: obj = logp * an, dlogp = an; logp_old is not used (the callers do not load it).
struct PolicyTerm {
    float obj;
    double dlogp;
};

template <int OBJ>
__device__ __forceinline__ PolicyTerm policy_term(float logp, float logp_old, float an,
                                                  const LossParams& p) {
    if constexpr (OBJ == OBJ_A2C) {
        return {logp * an, (double)an};
    } else {
        const float ratio = expf(logp - logp_old);
        const Surrogate sg = surrogate(ratio, an, p);
        return {sg.obj, (double)sg.dobj * (double)ratio};
    }
}

// The objective chosen at run time (p.objective).
__device__ __forceinline__ PolicyTerm policy_term(float logp, float logp_old, float an,
                                                  const LossParams& p) {
    return p.objective == OBJ_A2C ? policy_term<OBJ_A2C>(logp, logp_old, an, p)
                                  : policy_term<OBJ_PPO>(logp, logp_old, an, p);
}

// vf = (ret - v)^2, under value clip max(vf, (ret - (v_s + clamp(v - v_s, -eps, eps)))^2);
// dv = d(vf)/d(v).  v_s is read only under value clip.
struct ValueLoss {
    float vf, dv;
};

__device__ __forceinline__ ValueLoss value_loss(float v, float ret, float v_s,
                                                const LossParams& p) {
    float vf, dv;
    if (p.value_clip) {
        const float dlt = v - v_s;
        const float dcl = fminf(fmaxf(dlt, -p.eps_clip), p.eps_clip);
        const float vcl = v_s + dcl;
        const float e1 = ret - v, e2 = ret - vcl;
        const float vf1 = e1 * e1, vf2 = e2 * e2;
        const float g1 = -2.0f * e1;
        const float g2 = (dlt >= -p.eps_clip && dlt <= p.eps_clip) ? -2.0f * e2 : 0.0f;
        if (vf1 > vf2) {
            vf = vf1;
            dv = g1;
        } else if (vf2 > vf1) {
            vf = vf2;
            dv = g2;
        } else {
            vf = vf1;
            dv = 0.5f * g1 + 0.5f * g2;
        }
    } else {
        const float e1 = ret - v;
        vf = e1 * e1;
        dv = -2.0f * e1;
    }
    return {vf, dv};
}

// Loss terms (thread 0: loss, clip, vf, entropy) and the log-std gradient (strided over the
// block) of the Gaussian policy from the reduced sums [4 + A] = clip, vf, count, 0,
// d/dlog_std[A].  Every thread of the block calls it.  Acc is the type the per-dimension
// entropies are summed in: float is ppo_tail16_kernel's contract (at most 32 dimensions);
// gauss_finalize_kernel, which takes up to 64, sums in double and rounds once (an f32 running
// sum over 63 terms was off by 3.6 ulp, more than torch's sum(-1) ever is).
template <typename Acc = float>
__device__ __forceinline__ void gauss_finalize(const double* sums, int A, const float* log_std,
                                               float vf_coef, float ent_coef, double inv_b,
                                               float* losses, float* grad_log_std) {
    if (threadIdx.x == 0) {
        Acc ent_sum = 0;
        for (int a = 0; a < A; ++a) {
            const float sig = expf(log_std[a]);
            ent_sum += 1.4189385332046727f + logf(sig);  // f32(0.5 + 0.5*log(2*pi)) + log(scale)
        }
        const float ent = (float)ent_sum;
        const float clip = (float)(sums[0] * inv_b);
        const float vf = (float)(sums[1] * inv_b);
        losses[0] = clip + vf_coef * vf - ent_coef * ent;
        losses[1] = clip;
        losses[2] = vf;
        losses[3] = ent;
    }
    for (int a = threadIdx.x; a < A; a += blockDim.x)
        grad_log_std[a] = (float)(sums[4 + a] - (double)ent_coef);
}

}  // namespace tsrl
