// Continuous BCQ (tianshou/policy/imitation/bcq.py, utils/net/continuous.py:371-488).
//
// BCQ evaluates its decoder and critics on repeated rows: every observation R times (10 in
// learn, 100 in forward), each copy with a few own columns (a latent z or an action) appended.
// The reference materialises repeat + cat and runs a dense first layer over [G R, D + K], so
// the D-wide part of that layer is computed R times over identical rows.
//   group_linear_kernel   out[g R + k] = act(xs[g] Ws^T + xo[g R + k] Wo^T + bias), Ws = W[:, :D]
//                         and Wo = W[:, D:] read in place from the layer's one weight; neither
//                         the repeat nor the concat exists.  f32 operands on
//                         v_mfma_f32_32x32x2f32 (the targets feed an MSE against f32 critics).
// A workgroup is 4 waves over one tile of 32 groups and 128 output columns, a wave owns 32 x 32.
// Phase 1: S = xs_tile Ws_tile^T + bias over K = D in chunks of 64 staged through LDS (the xs
// chunk is shared by the four waves), rows / columns / k beyond the matrix zero-filled, so a last
// half-filled MFMA step multiplies zeros; four partial accumulators, folded once.  S then stays
// in the wave's 16 accumulator registers.
// Phase 2: the wave's Wo tile (32 x K, K <= 64) is loaded once into registers as MFMA B
// operands; for each k of its range the 32 rows {g R + k} of xo are read straight into A
// operands (adjacent k are adjacent rows: the lines stay in L1 / L2), the accumulator starts
// from S -- the add is free -- and act(acc) is stored as 32 rows of 128 contiguous bytes.
// Operand layout as fvp.hip: lane (c = l & 31, h = l >> 5) supplies A[c][k], B[k][c] for k =
// kk + 2 h, kk + 2 h + 1 of a four-k step; register r of the result is [rho(r) + 4 h][c].
// blockIdx.z = (triple, k split): an optional second (W, bias, out) serves the two target
// critics on the same inputs, and a small G splits the k range over workgroups that each
// recompute S (tsrl_group_linear states the rule).
//
// The per-element kernels (one lane per element or row; batch sums f64 in loss_sum.h's order, no
// float atomics): the VAE's reparameterisation and its loss, the perturbation with both
// gradients, the clipped-double-Q target with the max over each row's R samples, and the
// per-group argmax + action gather of forward.
#include "loss_sum.h"

#include <math.h>

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TPB = kLossTPB;  // 4 waves
constexpr int TG = 32;         // groups of a tile
constexpr int TH = 128;        // output columns of a workgroup, 32 per wave
constexpr int KC = 64;         // k of a staged chunk
constexpr int CS = KC + 2;     // its LDS stride: 8-byte reads of a row, conflict-free columns
constexpr int KMAX = TSRL_GROUP_LINEAR_MAX_OWN;
constexpr int KSTEPS = KMAX / 4;

__device__ __forceinline__ int rho(int r) { return (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct GroupArgs {
    const float *xs, *xo;
    const float* W[2];
    const float* bias[2];
    float* out[2];
    int64_t G, R, D, K, H, ldw;
    int nsplit, relu;
    int vec_xs, vec_w, vec_wo, vec_xo;  // 16-byte staging of xs / W rows, 8-byte Wo / xo pairs
};

// rows [row0, row0 + nrows) x k [k0, k0 + KC) of a row-major matrix (ld floats apart, `rows`
// x `kend` live) -> S[row][k] with stride CS; everything outside reads as zero.
__device__ __forceinline__ void stage(float* S, const float* __restrict__ M, int64_t ld,
                                      int64_t row0, int nrows, int64_t rows, int64_t k0,
                                      int64_t kend, bool vec, int t) {
    if (vec) {  // ld % 4 == 0 and kend % 4 == 0: a float4 is wholly inside or outside
        for (int i = t; i < nrows * (KC / 4); i += TPB) {
            const int row = i / (KC / 4), col = 4 * (i % (KC / 4));
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row0 + row < rows && k0 + col < kend)
                v = *reinterpret_cast<const float4*>(M + (row0 + row) * ld + k0 + col);
            *reinterpret_cast<float2*>(&S[row * CS + col]) = make_float2(v.x, v.y);
            *reinterpret_cast<float2*>(&S[row * CS + col + 2]) = make_float2(v.z, v.w);
        }
    } else {
        for (int i = t; i < nrows * KC; i += TPB) {
            const int row = i / KC, col = i % KC;
            float v = 0.f;
            if (row0 + row < rows && k0 + col < kend) v = M[(row0 + row) * ld + k0 + col];
            S[row * CS + col] = v;
        }
    }
}

// elements (k, k + 1) of a row of `n` floats, zero beyond; `vec`: the pair is 8-byte aligned and
// n is even
__device__ __forceinline__ float2 pair_at(const float* __restrict__ row, int k, int n, bool vec) {
    if (vec) {
        return k < n ? *reinterpret_cast<const float2*>(row + k) : make_float2(0.f, 0.f);
    }
    return make_float2(k < n ? row[k] : 0.f, k + 1 < n ? row[k + 1] : 0.f);
}

__global__ __launch_bounds__(TPB) void group_linear_kernel(GroupArgs a) {
    __shared__ __attribute__((aligned(16))) float xs_s[TG * CS];
    __shared__ __attribute__((aligned(16))) float w_s[TH * CS];
    const int t = threadIdx.x, w = t / kWave, lane = t & (kWave - 1);
    const int c = lane & 31, h = lane >> 5;
    const int trip = blockIdx.z / a.nsplit, split = blockIdx.z % a.nsplit;
    const float* __restrict__ W = a.W[trip];
    const float* __restrict__ bias = a.bias[trip];
    float* __restrict__ out = a.out[trip];
    const int64_t g0 = (int64_t)blockIdx.x * TG, hb = (int64_t)blockIdx.y * TH;
    const int64_t col = hb + 32 * w + c;  // this lane's output column (B operand line)
    const bool wave_live = hb + 32 * w < a.H;
    const int64_t per = (a.R + a.nsplit - 1) / a.nsplit;
    const int64_t kb = split * per, ke = kb + per < a.R ? kb + per : a.R;
    if (kb >= ke) return;  // a trailing part of the k split left without rows: the whole workgroup

    // -- phase 1: S = bias + xs_tile Ws_tile^T ------------------------------------------------
    // four accumulators over alternating k steps: the MFMAs of a chunk do not wait on each other,
    // and each partial sum is a quarter as long (one long f32 sum over D = 376 measured 3.9 x the
    // max-norm error of torch's f32 linear; four partial sums 0.7 x)
    f32x16 P[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) P[i][r] = 0.f;
    for (int64_t k0 = 0; k0 < a.D; k0 += KC) {
        __syncthreads();
        stage(xs_s, a.xs, a.D, g0, TG, a.G, k0, a.D, a.vec_xs, t);
        stage(w_s, W, a.ldw, hb, TH, a.H, k0, a.D, a.vec_w, t);
        __syncthreads();
        if (wave_live) {
            const float* pa = xs_s + c * CS + 2 * h;
            const float* pb = w_s + (32 * w + c) * CS + 2 * h;
#pragma unroll
            for (int kk = 0; kk < KC; kk += 4) {
                const float2 x = *reinterpret_cast<const float2*>(pa + kk);
                const float2 y = *reinterpret_cast<const float2*>(pb + kk);
                f32x16& acc = P[(kk / 4) & 3];
                acc = mfma(x.x, y.x, acc);
                acc = mfma(x.y, y.y, acc);
            }
        }
    }
    f32x16 S;
    const float bv = col < a.H ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) S[r] = ((P[0][r] + P[1][r]) + (P[2][r] + P[3][r])) + bv;
    if (!wave_live) return;  // no barrier below

    // -- phase 2: the own columns, k by k -------------------------------------------------------
    const int K = (int)a.K;
    const int nsteps = (K + 3) / 4;
    float2 b[KSTEPS];
    {
        const float* wo = W + (col < a.H ? col : 0) * a.ldw + a.D;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            b[s] = make_float2(0.f, 0.f);
            if (s < nsteps && col < a.H) b[s] = pair_at(wo, 4 * s + 2 * h, K, a.vec_wo);
        }
    }
    const bool row_live = g0 + c < a.G;  // this lane's A operand line
    const float* xo_row = a.xo + (row_live ? (g0 + c) * a.R : 0) * a.K;
    for (int64_t k = kb; k < ke; ++k) {
        float2 x[KSTEPS];
        const float* xr = xo_row + k * a.K;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            x[s] = make_float2(0.f, 0.f);
            if (s < nsteps && row_live) x[s] = pair_at(xr, 4 * s + 2 * h, K, a.vec_xo);
        }
        f32x16 acc = S;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            if (s < nsteps) {
                acc = mfma(x[s].x, b[s].x, acc);
                acc = mfma(x[s].y, b[s].y, acc);
            }
        }
        if (col < a.H) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t g = g0 + rho(r) + 4 * h;
                if (g < a.G) {
                    const float v = acc[r];
                    // torch's relu: NaN stays NaN
                    out[(g * a.R + k) * a.H + col] = a.relu ? (v < 0.f ? 0.f : v) : v;
                }
            }
        }
    }
}

// -- the per-element kernels ----------------------------------------------------------------
__global__ __launch_bounds__(TPB) void vae_sample_fwd_kernel(
    const float* __restrict__ mean, const float* __restrict__ log_std,
    const float* __restrict__ noise, int64_t n, float* __restrict__ z, float* __restrict__ std) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const float l = log_std[i];
    const float lc = l < -4.0f ? -4.0f : (l > 15.0f ? 15.0f : l);  // NaN stays NaN
    const float s = expf(lc);
    const float sn = s * noise[i];
    std[i] = s;
    z[i] = mean[i] + sn;
}

// g_mean = g_z + kl mean, g_log_std = (g_z noise + kl (std - 1 / std)) std inside the clamp
// (torch: lo <= x <= hi passes the gradient), 0 outside; kl = 1 / (2 n).
__global__ __launch_bounds__(TPB) void vae_sample_bwd_kernel(
    const float* __restrict__ g_z, const float* __restrict__ mean,
    const float* __restrict__ log_std, const float* __restrict__ noise,
    const float* __restrict__ std, int64_t n, double kl, float* __restrict__ g_mean,
    float* __restrict__ g_log_std) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const double g = (double)g_z[i], s = (double)std[i];
    const float l = log_std[i];
    g_mean[i] = (float)(g + kl * (double)mean[i]);
    const double gs = g * (double)noise[i] + kl * (s - 1.0 / s);
    g_log_std[i] = (l >= -4.0f && l <= 15.0f) ? (float)(gs * s) : 0.0f;
}

// s[0] = sum (act - recon)^2 over b A, s[1] = sum (-log std + (std^2 + mean^2 - 1) / 2) over b L.
struct VaeLosses {
    double bA, bL;
    float* loss;  // [3]: recon + KL / 2, recon, KL
    __device__ void operator()(const double* s) const {
        const double rec = s[0] / bA, kl = s[1] / bL;
        loss[0] = (float)(rec + kl / 2.0);
        loss[1] = (float)rec;
        loss[2] = (float)kl;
    }
};

__global__ __launch_bounds__(TPB) void vae_loss_kernel(
    const float* __restrict__ act, const float* __restrict__ recon,
    const float* __restrict__ mean, const float* __restrict__ std, int64_t b, int64_t A,
    int64_t L, float* __restrict__ g_recon, double* __restrict__ partials, VaeLosses fin) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double term[2] = {0.0, 0.0};
    if (r < b) {
        const double gs = 2.0 / fin.bA;
        for (int64_t j = 0; j < A; ++j) {
            const double d = (double)recon[r * A + j] - (double)act[r * A + j];
            term[0] += d * d;
            g_recon[r * A + j] = (float)(gs * d);
        }
        for (int64_t j = 0; j < L; ++j) {
            const double s = (double)std[r * L + j], m = (double)mean[r * L + j];
            term[1] += -log(s) + (s * s + m * m - 1.0) / 2.0;
        }
    }
    double s[2];
    block_sums<2>(term, s);
    losses_or_partials<2>(s, partials, fin);
}

// clamp(c tanh(logits) + act, +-m) with c = fl(phi max_action), torch's f32 order; logits row r
// starts at r * ls (ls = A, or 0: one row for all).
__device__ __forceinline__ float perturb_pre(float lg, float a, float c, float* th) {
#pragma clang fp contract(off)
    *th = tanhf(lg);
    const float p = c * *th;
    return p + a;
}

__global__ __launch_bounds__(TPB) void perturb_fwd_kernel(
    const float* __restrict__ logits, int64_t ls, const float* __restrict__ act, float c, float m,
    int64_t b, int64_t A, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= b * A) return;
    float th;
    const float v = perturb_pre(logits[(i / A) * ls + i % A], act[i], c, &th);
    out[i] = v < -m ? -m : (v > m ? m : v);  // NaN stays NaN
}

// One lane = one row.  ls = A: g_logits [b, A] element-wise.  ls = 0: g_logits [A] = the f64
// column sums over the rows, block_sums per column; beyond one workgroup the sums go to
// partials [A][nblk] and perturb_fold_kernel adds them in block order.
__global__ __launch_bounds__(TPB) void perturb_bwd_kernel(
    const float* __restrict__ g_out, const float* __restrict__ logits, int64_t ls,
    const float* __restrict__ act, float c, float m, int64_t b, int64_t A,
    float* __restrict__ g_act, float* __restrict__ g_logits, double* __restrict__ partials) {
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    for (int64_t j = 0; j < A; ++j) {
        double term = 0.0;
        if (r < b) {
            float th;
            const float v = perturb_pre(logits[r * ls + j], act[r * A + j], c, &th);
            const bool pass = v >= -m && v <= m;
            const float g = pass ? g_out[r * A + j] : 0.0f;
            g_act[r * A + j] = g;
            term = (double)g * (double)c * (1.0 - (double)th * (double)th);
            if (ls != 0) g_logits[r * A + j] = (float)term;
        }
        if (ls == 0) {
            double s;
            __syncthreads();  // the previous column's sums have been read
            block_sums<1>(&term, &s);
            if (threadIdx.x == 0) {
                if (gridDim.x == 1) g_logits[j] = (float)s;
                else partials[j * gridDim.x + blockIdx.x] = s;
            }
        }
    }
}

__global__ __launch_bounds__(TPB) void perturb_fold_kernel(const double* __restrict__ partials,
                                                           int64_t nblk, int64_t A,
                                                           float* __restrict__ g_logits) {
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (j >= A) return;
    double s = 0.0;
    for (int64_t i = 0; i < nblk; ++i) s += partials[j * nblk + i];
    g_logits[j] = (float)s;
}

// torch.max(a, b) / max over a dimension: a NaN is handed through.
__device__ __forceinline__ float max_nan(float a, float b) {
    return a != a ? a : (b != b ? b : (b > a ? b : a));
}

// bcq.py:161-172 in torch's f32 order, one lane = one row of the batch.
__global__ __launch_bounds__(TPB) void bcq_target_kernel(
    const float* __restrict__ q1, const float* __restrict__ q2, const float* __restrict__ rew,
    const float* __restrict__ done, float lmbda, float one_m_lmbda, float gamma, int64_t b,
    int64_t R, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int64_t r = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (r >= b) return;
    float best = 0.f;
    for (int64_t k = 0; k < R; ++k) {
        const float x = q1[r * R + k], y = q2[r * R + k];
        const float lo = lmbda * min_nan(x, y);
        const float hi = one_m_lmbda * max_nan(x, y);
        const float v = lo + hi;
        best = k == 0 ? v : max_nan(best, v);
    }
    const float cg = (1.0f - done[r]) * gamma;
    const float t = cg * best;
    out[r] = rew[r] + t;
}

// One lane = one group: the first index of the maximum of q over its R rows (torch.argmax: a
// NaN counts as the maximum), then that action row.
__global__ __launch_bounds__(TPB) void bcq_select_kernel(
    const float* __restrict__ q, const float* __restrict__ act, int64_t G, int64_t R, int64_t A,
    float* __restrict__ out, int64_t* __restrict__ index) {
    const int64_t g = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (g >= G) return;
    int64_t bi = 0;
    float best = q[g * R];
    for (int64_t k = 1; k < R; ++k) {
        const float v = q[g * R + k];
        if (best == best && (v > best || v != v)) {
            best = v;
            bi = k;
        }
    }
    for (int64_t j = 0; j < A; ++j) out[g * A + j] = act[(g * R + bi) * A + j];
    if (index) index[g] = bi;
}

inline unsigned blocks_of(int64_t n, int64_t per) { return (unsigned)((n + per - 1) / per); }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
constexpr int64_t kMaxRows = (int64_t)1 << 31;

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_group_linear_splits(int64_t G, int64_t R, int64_t D, int64_t K, int64_t H,
                                        int64_t n_out) {
    // The k split.  Without one a launch has wg = ceil(G / 32) ceil(H / 128) n_out workgroups,
    // each computing S (about D / 4 MFMA steps, twice that with its staging) and then R own
    // passes (K / 4 steps and a 32 x 32 store, about 8 steps' worth).  n parts make n wg
    // workgroups of S + ceil(R / n) passes each, run in ceil(n wg / CUs) rounds; take the n with
    // the least rounds x work per workgroup, the smallest such n.  A batch of 256 keeps every CU
    // busy with few parts; acting on a handful of observations with R = 100 splits k finely.
    if (G < 1 || R < 1 || H < 1 || n_out < 1) return 1;
    const int64_t wg = ((G + TG - 1) / TG) * ((H + TH - 1) / TH) * n_out, cus = n_cus();
    const int64_t cs = 2 * ((D + 3) / 4), co = (K + 3) / 4 + 8;
    int64_t best = 1, best_cost = -1;
    for (int64_t n = 1; n <= R && n * wg <= 65535; ++n) {
        const int64_t cost = ((n * wg + cus - 1) / cus) * (cs + ((R + n - 1) / n) * co);
        if (best_cost < 0 || cost < best_cost) {
            best = n;
            best_cost = cost;
        }
    }
    return (int)best;
}

extern "C" int tsrl_group_linear(const float* xs, const float* xo, const float* W, int64_t ldw,
                                 const float* bias, float* out, const float* W2,
                                 const float* bias2, float* out2, int64_t G, int64_t R, int64_t D,
                                 int64_t K, int64_t H, int relu, void* stream) {
    TSRL_CHECK_ARG(G >= 1 && R >= 1 && D >= 1 && K >= 1 && H >= 1 && ldw >= D + K,
                   "tsrl_group_linear: need G, R, D, K, H >= 1 and ldw >= D + K");
    TSRL_CHECK_ARG(xs && xo && W && bias && out, "tsrl_group_linear: null pointer");
    TSRL_CHECK_ARG((W2 != nullptr) == (bias2 != nullptr) && (W2 != nullptr) == (out2 != nullptr),
                   "tsrl_group_linear: the second output needs W2, bias2 and out2");
    if (K > KMAX || G > kMaxRows / R || G * R > kMaxRows / H || (H + TH - 1) / TH > 65535) {
        set_error("tsrl_group_linear: K = %lld exceeds the %d own columns staged per row, or "
                  "G R H exceeds 2^31", (long long)K, KMAX);
        return TSRL_ERR_GROUP_LINEAR_SHAPE;
    }
    const int n_out = W2 ? 2 : 1;
    GroupArgs a;
    a.xs = xs;
    a.xo = xo;
    a.W[0] = W;
    a.W[1] = W2 ? W2 : W;
    a.bias[0] = bias;
    a.bias[1] = W2 ? bias2 : bias;
    a.out[0] = out;
    a.out[1] = W2 ? out2 : out;
    a.G = G, a.R = R, a.D = D, a.K = K, a.H = H, a.ldw = ldw;
    a.nsplit = tsrl_group_linear_splits(G, R, D, K, H, n_out);
    a.relu = relu != 0;
    // vector loads only where every address they touch allows them (tsrl_noisy_weights' rule)
    a.vec_xs = D % 4 == 0 && aligned16(xs);
    a.vec_w = D % 4 == 0 && ldw % 4 == 0 && aligned16(W) && aligned16(a.W[1]);
    a.vec_wo = K % 2 == 0 && D % 2 == 0 && ldw % 2 == 0 && aligned8(W) && aligned8(a.W[1]);
    a.vec_xo = K % 2 == 0 && aligned8(xo);
    const dim3 grid(blocks_of(G, TG), blocks_of(H, TH), (unsigned)(n_out * a.nsplit));
    hipLaunchKernelGGL(group_linear_kernel, grid, dim3(TPB), 0, as_stream(stream), a);
    TSRL_LAUNCH_CHECK("tsrl_group_linear");
    return 0;
}

extern "C" int tsrl_bcq_vae_sample_fwd(const float* mean, const float* log_std,
                                       const float* noise, int64_t n, float* z, float* std,
                                       void* stream) {
    TSRL_CHECK_ARG(n >= 1 && n < kMaxRows * TPB, "tsrl_bcq_vae_sample_fwd: need n >= 1");
    TSRL_CHECK_ARG(mean && log_std && noise && z && std, "tsrl_bcq_vae_sample_fwd: null pointer");
    hipLaunchKernelGGL(vae_sample_fwd_kernel, dim3(blocks_of(n, TPB)), dim3(TPB), 0,
                       as_stream(stream), mean, log_std, noise, n, z, std);
    TSRL_LAUNCH_CHECK("tsrl_bcq_vae_sample_fwd");
    return 0;
}

extern "C" int tsrl_bcq_vae_sample_bwd(const float* g_z, const float* mean, const float* log_std,
                                       const float* noise, const float* std, int64_t n,
                                       float* g_mean, float* g_log_std, void* stream) {
    TSRL_CHECK_ARG(n >= 1 && n < kMaxRows * TPB, "tsrl_bcq_vae_sample_bwd: need n >= 1");
    TSRL_CHECK_ARG(g_z && mean && log_std && noise && std && g_mean && g_log_std,
                   "tsrl_bcq_vae_sample_bwd: null pointer");
    hipLaunchKernelGGL(vae_sample_bwd_kernel, dim3(blocks_of(n, TPB)), dim3(TPB), 0,
                       as_stream(stream), g_z, mean, log_std, noise, std, n,
                       0.5 / (double)n, g_mean, g_log_std);
    TSRL_LAUNCH_CHECK("tsrl_bcq_vae_sample_bwd");
    return 0;
}

extern "C" int tsrl_bcq_vae_loss_fwd_bwd(const float* act, const float* recon, const float* mean,
                                         const float* std, int64_t b, int64_t A, int64_t L,
                                         float* g_recon, double* partials, float* loss,
                                         void* stream) {
    TSRL_CHECK_ARG(b >= 1 && A >= 1 && L >= 1 && b < kMaxRows / A && b < kMaxRows / L,
                   "tsrl_bcq_vae_loss_fwd_bwd: need b, A, L >= 1 and b A, b L < 2^31");
    TSRL_CHECK_ARG(act && recon && mean && std && g_recon && loss,
                   "tsrl_bcq_vae_loss_fwd_bwd: null pointer");
    const hipStream_t st = as_stream(stream);
    const VaeLosses fin{(double)b * (double)A, (double)b * (double)L, loss};
    return launch_loss<2>("tsrl_bcq_vae_loss_fwd_bwd", b, partials, fin, st, [&](unsigned nblk) {
        hipLaunchKernelGGL(vae_loss_kernel, dim3(nblk), dim3(TPB), 0, st, act, recon, mean, std,
                           b, A, L, g_recon, partials, fin);
    });
}

extern "C" int tsrl_bcq_perturb_fwd(const float* logits, int64_t logits_stride, const float* act,
                                    double phi, double max_action, int64_t b, int64_t A,
                                    float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && A >= 1 && b < kMaxRows / A,
                   "tsrl_bcq_perturb_fwd: need b, A >= 1 and b A < 2^31");
    TSRL_CHECK_ARG(logits_stride == 0 || logits_stride == A,
                   "tsrl_bcq_perturb_fwd: logits_stride is A or 0");
    TSRL_CHECK_ARG(logits && act && out, "tsrl_bcq_perturb_fwd: null pointer");
    hipLaunchKernelGGL(perturb_fwd_kernel, dim3(blocks_of(b * A, TPB)), dim3(TPB), 0,
                       as_stream(stream), logits, logits_stride, act, (float)(phi * max_action),
                       (float)max_action, b, A, out);
    TSRL_LAUNCH_CHECK("tsrl_bcq_perturb_fwd");
    return 0;
}

extern "C" int tsrl_bcq_perturb_bwd(const float* g_out, const float* logits,
                                    int64_t logits_stride, const float* act, double phi,
                                    double max_action, int64_t b, int64_t A, float* g_act,
                                    float* g_logits, double* partials, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && A >= 1 && b < kMaxRows / A,
                   "tsrl_bcq_perturb_bwd: need b, A >= 1 and b A < 2^31");
    TSRL_CHECK_ARG(logits_stride == 0 || logits_stride == A,
                   "tsrl_bcq_perturb_bwd: logits_stride is A or 0");
    TSRL_CHECK_ARG(g_out && logits && act && g_act && g_logits,
                   "tsrl_bcq_perturb_bwd: null pointer");
    const int64_t nblk = loss_blocks(b);
    const bool fold = logits_stride == 0 && nblk > 1;
    TSRL_CHECK_ARG(!fold || partials, "tsrl_bcq_perturb_bwd: b > %d at stride 0 needs partials",
                   TPB);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(perturb_bwd_kernel, dim3((unsigned)nblk), dim3(TPB), 0, st, g_out, logits,
                       logits_stride, act, (float)(phi * max_action), (float)max_action, b, A,
                       g_act, g_logits, partials);
    TSRL_LAUNCH_CHECK("tsrl_bcq_perturb_bwd");
    if (fold) {
        hipLaunchKernelGGL(perturb_fold_kernel, dim3(blocks_of(A, TPB)), dim3(TPB), 0, st,
                           partials, nblk, A, g_logits);
        TSRL_LAUNCH_CHECK("tsrl_bcq_perturb_bwd (fold)");
    }
    return 0;
}

extern "C" int tsrl_bcq_target(const float* q1, const float* q2, const float* rew,
                               const float* done, double lmbda, double gamma, int64_t b,
                               int64_t R, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 1 && R >= 1 && b < kMaxRows / R,
                   "tsrl_bcq_target: need b, R >= 1 and b R < 2^31");
    TSRL_CHECK_ARG(q1 && q2 && rew && done && out, "tsrl_bcq_target: null pointer");
    hipLaunchKernelGGL(bcq_target_kernel, dim3(blocks_of(b, TPB)), dim3(TPB), 0,
                       as_stream(stream), q1, q2, rew, done, (float)lmbda, (float)(1.0 - lmbda),
                       (float)gamma, b, R, out);
    TSRL_LAUNCH_CHECK("tsrl_bcq_target");
    return 0;
}

extern "C" int tsrl_bcq_select_act(const float* q, const float* act, int64_t G, int64_t R,
                                   int64_t A, float* out, int64_t* index, void* stream) {
    TSRL_CHECK_ARG(G >= 1 && R >= 1 && A >= 1 && G < kMaxRows / R && G * R < kMaxRows / A,
                   "tsrl_bcq_select_act: need G, R, A >= 1 and G R A < 2^31");
    TSRL_CHECK_ARG(q && act && out, "tsrl_bcq_select_act: null pointer");
    hipLaunchKernelGGL(bcq_select_kernel, dim3(blocks_of(G, TPB)), dim3(TPB), 0,
                       as_stream(stream), q, act, G, R, A, out, index);
    TSRL_LAUNCH_CHECK("tsrl_bcq_select_act");
    return 0;
}
