// RainbowPolicy's small passes (tianshou/policy/modelfree/rainbow.py, utils/net/discrete.py
// NoisyLinear, utils/net/common.py Net's dueling combine, examples/atari Rainbow's head).
//   noisy_eps:      f(x) = sign(x) sqrt|x| over the staged normal draws of a whole network
//                   (discrete.py:361-367), bit for bit torch's x.sign().mul_(x.abs().sqrt_());
//   noisy_weights:  mu + sigma * eps of every noisy layer of one or more networks in one launch
//                   (discrete.py:371-374), each product and sum rounded to f32 on its own;
//   noisy_grads:    the sigma gradients of one layer from the effective weight's gradient;
//   dueling_fwd/bwd: q - mean_a q + v and the softmax over the atoms (common.py:276-284),
//                   one workgroup per batch row, the row in LDS, f64 arithmetic on f32 inputs.
// The noisy kernels are memory-bound element-wise passes: 16-byte accesses where a layer's
// pointers and row length allow (parameters are views packed into a flat buffer, so a layer
// after one with an odd element count is only 4-byte aligned), scalar otherwise.
#include "tsrl_common.h"

// every f32 product and sum below is rounded on its own, as torch's one-op-per-kernel
// formulation rounds them: no FMA contraction anywhere in this file
#pragma clang fp contract(off)

namespace tsrl {
namespace {

constexpr int TPB = 256;
constexpr int NW = TPB / kWave;
constexpr int kMaxBlocksX = 2048;
constexpr int64_t kMaxRow = TSRL_DUELING_MAX_ROW;  // floats of one [A, N] row staged in LDS

__device__ __forceinline__ float noisy_f(float x) {
    const float s = (float)((0.0f < x) - (x < 0.0f));  // torch's sign: 0 for +-0 and NaN
    return s * sqrtf(fabsf(x));
}

__global__ __launch_bounds__(TPB) void noisy_eps_kernel(const float* __restrict__ x, int64_t n,
                                                        float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * TPB)
        out[i] = noisy_f(x[i]);
}

// W[o][i] = mu[o][i] + sigma[o][i] * (eq[o] * ep[i]) over one layer's [out, in] block, the
// workgroups of grid row blockIdx.y striding over it.  VEC: four consecutive i of one row.
template <bool VEC>
__device__ __forceinline__ void noisy_weight_block(const tsrl_noisy_layer& L) {
    const int64_t in = L.in, nel = L.in * L.out;
    const int64_t start = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * TPB;
    if (VEC) {
        const float4* mu4 = reinterpret_cast<const float4*>(L.mu_w);
        const float4* sg4 = reinterpret_cast<const float4*>(L.sigma_w);
        float4* w4 = reinterpret_cast<float4*>(L.w_eff);
        for (int64_t e = start; e < nel / 4; e += step) {
            const int64_t o = (e * 4) / in, i = (e * 4) - o * in;  // in % 4 == 0: one row
            const float q = L.eps_q[o];
            const float4 m = mu4[e], s = sg4[e];
            float4 r;
            r.x = m.x + s.x * (q * L.eps_p[i]);
            r.y = m.y + s.y * (q * L.eps_p[i + 1]);
            r.z = m.z + s.z * (q * L.eps_p[i + 2]);
            r.w = m.w + s.w * (q * L.eps_p[i + 3]);
            w4[e] = r;
        }
    } else {
        for (int64_t e = start; e < nel; e += step) {
            const int64_t o = e / in, i = e - o * in;
            L.w_eff[e] = L.mu_w[e] + L.sigma_w[e] * (L.eps_q[o] * L.eps_p[i]);
        }
    }
    for (int64_t o = start; o < L.out; o += step)
        L.b_eff[o] = L.mu_b[o] + L.sigma_b[o] * L.eps_q[o];
}

__global__ __launch_bounds__(TPB) void noisy_weights_kernel(
    const tsrl_noisy_layer* __restrict__ table) {
    const tsrl_noisy_layer L = table[blockIdx.y];
    if ((int64_t)blockIdx.x * TPB >= L.in * L.out && (int64_t)blockIdx.x * TPB >= L.out) return;
    const bool vec = (L.in & 3) == 0 && aligned16(L.mu_w) && aligned16(L.sigma_w) &&
                     aligned16(L.w_eff);
    if (vec)
        noisy_weight_block<true>(L);
    else
        noisy_weight_block<false>(L);
}

// g_sigma_w[o][i] = gw[o][i] * (eq[o] * ep[i]), g_sigma_b[o] = gb[o] * eq[o].
template <bool VEC>
__global__ __launch_bounds__(TPB) void noisy_grads_kernel(
    const float* __restrict__ gw, const float* __restrict__ gb, const float* __restrict__ ep,
    const float* __restrict__ eq, int64_t in, int64_t out, float* __restrict__ g_sigma_w,
    float* __restrict__ g_sigma_b) {
    const int64_t nel = in * out;
    const int64_t start = (int64_t)blockIdx.x * TPB + threadIdx.x;
    const int64_t step = (int64_t)gridDim.x * TPB;
    if (VEC) {
        const float4* g4 = reinterpret_cast<const float4*>(gw);
        float4* s4 = reinterpret_cast<float4*>(g_sigma_w);
        for (int64_t e = start; e < nel / 4; e += step) {
            const int64_t o = (e * 4) / in, i = (e * 4) - o * in;
            const float q = eq[o];
            const float4 g = g4[e];
            float4 r;
            r.x = g.x * (q * ep[i]);
            r.y = g.y * (q * ep[i + 1]);
            r.z = g.z * (q * ep[i + 2]);
            r.w = g.w * (q * ep[i + 3]);
            s4[e] = r;
        }
    } else {
        for (int64_t e = start; e < nel; e += step) {
            const int64_t o = e / in, i = e - o * in;
            g_sigma_w[e] = gw[e] * (eq[o] * ep[i]);
        }
    }
    for (int64_t o = start; o < out; o += step) g_sigma_b[o] = gb[o] * eq[o];
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// Dynamic LDS of both dueling kernels: doubles first (8-byte aligned), then the f32 rows.
extern __shared__ __attribute__((aligned(16))) double dlds[];

// One batch row.  LDS: m[k] = v[k] - mean_a q[a][k] (N doubles), then the q row (A N floats).
// Threads over k build m; then either every thread writes q + m, or wave w takes the actions
// w, w + NW, ... and normalises exp(l - max l) over its lanes.
__global__ __launch_bounds__(TPB) void dueling_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ v, int64_t A, int64_t N, int softmax,
    float* __restrict__ out) {
    double* s_m = dlds;
    float* s_q = reinterpret_cast<float*>(dlds + N);
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x, nel = A * N;
    const float* q_row = q + r * nel;
    float* o_row = out + r * nel;
    for (int64_t f = t; f < nel; f += TPB) s_q[f] = q_row[f];
    __syncthreads();
    const double inv_a = 1.0 / (double)A;
    for (int64_t k = t; k < N; k += TPB) {
        double s = 0.0;
        for (int64_t a = 0; a < A; ++a) s += (double)s_q[a * N + k];
        s_m[k] = (double)v[r * N + k] - s * inv_a;
    }
    __syncthreads();
    if (!softmax) {
        for (int64_t f = t; f < nel; f += TPB) o_row[f] = (float)((double)s_q[f] + s_m[f % N]);
        return;
    }
    for (int64_t a = wv; a < A; a += NW) {
        const float* x = s_q + a * N;
        double mx = -INFINITY;
        for (int64_t k = lane; k < N; k += kWave) mx = fmax(mx, (double)x[k] + s_m[k]);
        mx = wave_max(mx);
        double sum = 0.0;
        for (int64_t k = lane; k < N; k += kWave) sum += exp((double)x[k] + s_m[k] - mx);
        sum = wave_sum(sum);
        for (int64_t k = lane; k < N; k += kWave)
            o_row[a * N + k] = (float)(exp((double)x[k] + s_m[k] - mx) / sum);
    }
}

// One batch row.  LDS: dot[a] = sum_k g p (A doubles, softmax only), then the g row and, with
// softmax, the p row (A N floats each).  g_l = p (g - dot[a]) or g; threads over k sum it
// over the actions for g_v and subtract that sum's mean for g_q.
__global__ __launch_bounds__(TPB) void dueling_bwd_kernel(
    const float* __restrict__ g_out, const float* __restrict__ out, int64_t A, int64_t N,
    int softmax, float* __restrict__ g_q, float* __restrict__ g_v) {
    double* s_dot = dlds;
    float* s_g = reinterpret_cast<float*>(dlds + A);
    float* s_p = s_g + A * N;
    const int t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int64_t r = blockIdx.x, nel = A * N;
    for (int64_t f = t; f < nel; f += TPB) {
        s_g[f] = g_out[r * nel + f];
        if (softmax) s_p[f] = out[r * nel + f];
    }
    __syncthreads();
    if (softmax) {
        for (int64_t a = wv; a < A; a += NW) {
            double d = 0.0;
            for (int64_t k = lane; k < N; k += kWave)
                d += (double)s_g[a * N + k] * (double)s_p[a * N + k];
            d = wave_sum(d);
            if (lane == 0) s_dot[a] = d;
        }
        __syncthreads();
    }
    const double inv_a = 1.0 / (double)A;
    for (int64_t k = t; k < N; k += TPB) {
        double s = 0.0;
        for (int64_t a = 0; a < A; ++a) {
            const double g = (double)s_g[a * N + k];
            s += softmax ? (double)s_p[a * N + k] * (g - s_dot[a]) : g;
        }
        g_v[r * N + k] = (float)s;
        const double mean = s * inv_a;
        for (int64_t a = 0; a < A; ++a) {
            const double g = (double)s_g[a * N + k];
            const double gl = softmax ? (double)s_p[a * N + k] * (g - s_dot[a]) : g;
            g_q[r * nel + a * N + k] = (float)(gl - mean);
        }
    }
}

inline unsigned blocks_for(int64_t work_items) {
    const int64_t nb = (work_items + TPB - 1) / TPB;
    return (unsigned)(nb < 1 ? 1 : (nb > kMaxBlocksX ? kMaxBlocksX : nb));
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_noisy_eps(const float* x, int64_t n, float* out, void* stream) {
    TSRL_CHECK_ARG(n >= 0, "tsrl_noisy_eps: need n >= 0");
    if (n == 0) return 0;
    TSRL_CHECK_ARG(x && out, "tsrl_noisy_eps: null pointer");
    hipLaunchKernelGGL(noisy_eps_kernel, dim3(blocks_for(n)), dim3(TPB), 0, as_stream(stream), x,
                       n, out);
    TSRL_LAUNCH_CHECK("tsrl_noisy_eps");
    return 0;
}

extern "C" int tsrl_noisy_weights(const tsrl_noisy_layer* table, int64_t n_layers,
                                  int64_t max_elems, void* stream) {
    TSRL_CHECK_ARG(n_layers >= 0 && n_layers <= 65535 && max_elems >= 0,
                   "tsrl_noisy_weights: need 0 <= n_layers <= 65535 and max_elems >= 0");
    if (n_layers == 0 || max_elems == 0) return 0;
    TSRL_CHECK_ARG(table, "tsrl_noisy_weights: null table");
    // a workgroup covers up to 4 TPB elements of a vectorised layer per stride; sizing the
    // grid row for the scalar path of the largest layer keeps every path inside one stride
    // up to kMaxBlocksX workgroups, and strides beyond
    hipLaunchKernelGGL(noisy_weights_kernel, dim3(blocks_for((max_elems + 3) / 4),
                                                  (unsigned)n_layers), dim3(TPB), 0,
                       as_stream(stream), table);
    TSRL_LAUNCH_CHECK("tsrl_noisy_weights");
    return 0;
}

extern "C" int tsrl_noisy_grads(const float* gw, const float* gb, const float* eps_p,
                                const float* eps_q, int64_t in, int64_t out, float* g_sigma_w,
                                float* g_sigma_b, void* stream) {
    TSRL_CHECK_ARG(in >= 0 && out >= 0, "tsrl_noisy_grads: need in >= 0 and out >= 0");
    if (in == 0 || out == 0) return 0;
    TSRL_CHECK_ARG(gw && gb && eps_p && eps_q && g_sigma_w && g_sigma_b,
                   "tsrl_noisy_grads: null pointer");
    const bool vec = (in & 3) == 0 && aligned16(gw) && aligned16(g_sigma_w);
    const dim3 grid(blocks_for(vec ? in * out / 4 : in * out));
    if (vec)
        hipLaunchKernelGGL(noisy_grads_kernel<true>, grid, dim3(TPB), 0, as_stream(stream), gw,
                           gb, eps_p, eps_q, in, out, g_sigma_w, g_sigma_b);
    else
        hipLaunchKernelGGL(noisy_grads_kernel<false>, grid, dim3(TPB), 0, as_stream(stream), gw,
                           gb, eps_p, eps_q, in, out, g_sigma_w, g_sigma_b);
    TSRL_LAUNCH_CHECK("tsrl_noisy_grads");
    return 0;
}

extern "C" int tsrl_dueling_fwd(const float* q, const float* v, int64_t b, int64_t num_actions,
                                int64_t n, int softmax, float* out, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1,
                   "tsrl_dueling_fwd: need 0 <= b < 2^31, num_actions >= 1 and n >= 1");
    if (num_actions > kMaxRow || n > kMaxRow || num_actions * n > kMaxRow) {
        set_error("tsrl_dueling_fwd: num_actions * n = %lld exceeds the LDS row of %d floats",
                  (long long)(num_actions * n), (int)kMaxRow);
        return TSRL_ERR_DUELING_ROW;
    }
    if (b == 0) return 0;
    TSRL_CHECK_ARG(q && v && out, "tsrl_dueling_fwd: null pointer");
    const size_t lds = (size_t)n * sizeof(double) + (size_t)(num_actions * n) * sizeof(float);
    hipLaunchKernelGGL(dueling_fwd_kernel, dim3((unsigned)b), dim3(TPB), lds, as_stream(stream),
                       q, v, num_actions, n, softmax, out);
    TSRL_LAUNCH_CHECK("tsrl_dueling_fwd");
    return 0;
}

extern "C" int tsrl_dueling_bwd(const float* g_out, const float* out, int64_t b,
                                int64_t num_actions, int64_t n, int softmax, float* g_q,
                                float* g_v, void* stream) {
    TSRL_CHECK_ARG(b >= 0 && b < ((int64_t)1 << 31) && num_actions >= 1 && n >= 1,
                   "tsrl_dueling_bwd: need 0 <= b < 2^31, num_actions >= 1 and n >= 1");
    if (num_actions > kMaxRow || n > kMaxRow || num_actions * n > kMaxRow) {
        set_error("tsrl_dueling_bwd: num_actions * n = %lld exceeds the LDS row of %d floats",
                  (long long)(num_actions * n), (int)kMaxRow);
        return TSRL_ERR_DUELING_ROW;
    }
    if (b == 0) return 0;
    TSRL_CHECK_ARG(g_out && g_q && g_v && (!softmax || out), "tsrl_dueling_bwd: null pointer");
    const size_t lds = (size_t)num_actions * sizeof(double) +
                       (size_t)(num_actions * n) * sizeof(float) * (softmax ? 2 : 1);
    hipLaunchKernelGGL(dueling_bwd_kernel, dim3((unsigned)b), dim3(TPB), lds, as_stream(stream),
                       g_out, out, num_actions, n, softmax, g_q, g_v);
    TSRL_LAUNCH_CHECK("tsrl_dueling_bwd");
    return 0;
}
