// Fisher-vector product of the diagonal-Gaussian MLP actor and the conjugate-gradient step of
// NPGPolicy / TRPOPolicy (tianshou/policy/modelfree/npg.py:132-181).
//
// For actor = Linear(D,64)-Tanh-Linear(64,64)-Tanh-Linear(64,A) with a state-independent
// log-std, the Hessian of KL(old || new).mean() at new = old is the Fisher matrix, so the
// reference's double backward is one tangent forward and one ordinary backward (include/tsrl.h
// states the operator).  Kernels:
//   fvp_kernel<true>   tsrl_fvp_prepare: h1, h2 of the n rows, row-major into the workspace
//   fvp_kernel<false>  tsrl_fvp_apply, main: per 64-row tile the tangent pass, the backward
//                      chain and the layer-2/3 weight gradients (phase 1), then dW1 = dz1^T X
//                      from a 64 x 384 X panel resident in LDS (phase 2); one partial per workgroup
//   fvp_fold_kernel    sums the partials in workgroup order, adds damping v, leaves p.z partials
//   cg_init / cg_step  the CG recurrences on device vectors, scalars in f64, early stop as a flag
//
// Every product is v_mfma_f32_32x32x2f32 on f32 operands (CG divides by p.Fp: no reduced
// precision).  A workgroup is 4 waves; a 64 x 64 result is four 32 x 32 tiles, one per wave.
// Operands are read from LDS: lane (c = l & 31, h = l >> 5) supplies A[i = c][k] and B[k][j = c]
// for k = kk + 2h, kk + 2h + 1 of each four-k step (two MFMAs).  Activations are kept row-major
// [row][feature] with stride 66 (8-byte reads of a row, conflict-free reads of a column), so the
// same array serves as the B operand of the chain (k = feature) and, read by columns, as an
// operand of the weight gradients (k = row).  The C layout (mlp.hip: register r of lane (c, h)
// is element [rho(r) + 4h][c]) is written back to LDS once per product.
//
// No atomics anywhere: partials are folded in a fixed order, two calls are bitwise equal.
#include "tsrl_common.h"

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int H = 64;            // hidden width
constexpr int AMAX = 32;         // action dims padded to one MFMA tile
constexpr int TR = 64;           // rows of a tile
constexpr int TPB = 256;         // 4 waves
constexpr int AS = 66;           // stride of a [64][64] activation / weight array in LDS
constexpr int GS = 34;           // stride of g [64][32]
constexpr int KC = 32;           // K chunk of the first layer
constexpr int CS = 34;           // stride of a staged chunk [64][32]
constexpr int PANEL = 384;       // X columns resident in phase 2
constexpr int XSTR = PANEL + 2;  // their LDS stride (2 mod 32, as CS)
constexpr int NKT = PANEL / 32 / 2;  // dW1 column tiles per wave

// LDS map (floats).  Phase 1:
constexpr int L_W2 = 0, L_V2 = L_W2 + H * AS, L_W3 = L_V2 + H * AS, L_V3 = L_W3 + AMAX * AS,
              L_H1 = L_V3 + AMAX * AS, L_H2 = L_H1 + TR * AS, L_TA = L_H2 + TR * AS,
              L_TB = L_TA + TR * AS,       // also the V1 / W1 chunk ring [2][64][CS]
              L_G = L_TB + 2 * H * CS, L_XC = L_G + TR * GS, L_VEC = L_XC + 2 * TR * CS,
              L_END1 = L_VEC + 2 * H + 2 * AMAX;
constexpr int V_C1 = 0, V_C2 = H, V_C3 = 2 * H, V_IV = 2 * H + AMAX;
// Phase 2 (over the same memory):
constexpr int L_XS = 0, L_DZ = L_XS + TR * XSTR, L_END2 = L_DZ + TR * AS;
constexpr int L_END = L_END1 > L_END2 ? L_END1 : L_END2;
static_assert(L_END * 4 <= 163840, "fvp LDS");
static_assert(2 * H * CS >= TR * AS, "chunk ring covers TB");

__device__ __forceinline__ int rho(int r) { return (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
    return z;
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// Operand fetchers: element pair (k, k + 1) of line `line`.
struct RowMajor {  // M[line][k]
    const float* s;
    __device__ __forceinline__ float2 operator()(int k) const {
        return *reinterpret_cast<const float2*>(s + k);
    }
};
struct ColMajor {  // M[k][line]
    const float* s;
    int stride;
    __device__ __forceinline__ float2 operator()(int k) const {
        return make_float2(s[k * stride], s[(k + 1) * stride]);
    }
};
__device__ __forceinline__ RowMajor rowm(const float* S, int stride, int line) {
    return RowMajor{S + line * stride};
}
__device__ __forceinline__ ColMajor colm(const float* S, int stride, int line) {
    return ColMajor{S + line, stride};
}

// acc[i][j] += sum_{k < K} A[i][k] B[k][j], K % 4 == 0.
template <class FA, class FB>
__device__ __forceinline__ void gemm32(f32x16& acc, int K, int h, FA fa, FB fb) {
#pragma unroll 4
    for (int kk = 0; kk < K; kk += 4) {
        const float2 a = fa(kk + 2 * h), b = fb(kk + 2 * h);
        acc = mfma(a.x, b.x, acc);
        acc = mfma(a.y, b.y, acc);
    }
}

// C tile (it, jt) -> S[32 jt + c][32 it + rho(r) + 4h] = f(acc, row, feature): the transposed
// products' results land row-major.
template <class F>
__device__ __forceinline__ void put_tile(float* S, int stride, const f32x16& acc, int it, int jt,
                                         int c, int h, F f) {
    const int row = 32 * jt + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ft = 32 * it + rho(r) + 4 * h;
        S[row * stride + ft] = f(acc[r], row, ft);
    }
}

__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int nw = blockDim.x / kWave;
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += sh[i];
    return s;
}

struct Net {
    const float *w1, *b1, *w2, *b2, *w3, *b3, *log_std;
    int64_t off_sigma, off_w1, off_b1, off_w2, off_b2, off_w3, off_b3, n_params;
};

// Workspace: p.z partials first (tsrl_cg_step reads them from the workspace's start).
struct Ws {
    double* pz;
    float *h1, *h2, *dz1, *part;
    int64_t bytes;
};
__host__ __device__ inline int64_t n_params_of(int64_t D, int64_t A) {
    return A + H * D + H + H * H + H + A * H + A;
}
inline int64_t fold_blocks(int64_t P) { return (P + TPB - 1) / TPB; }
inline int grid_of(int64_t n) {
    const int64_t tiles = (n + TR - 1) / TR;
    return (int)(tiles < n_cus() ? tiles : n_cus());
}
inline Ws carve(void* ws, int64_t n, int64_t D, int64_t A) {
    const int64_t P = n_params_of(D, A);
    char* p = static_cast<char*>(ws);
    Ws w;
    w.pz = reinterpret_cast<double*>(p);
    p += (fold_blocks(P) * 8 + 15) / 16 * 16;
    w.h1 = reinterpret_cast<float*>(p);
    p += n * H * 4;
    w.h2 = reinterpret_cast<float*>(p);
    p += n * H * 4;
    w.dz1 = reinterpret_cast<float*>(p);
    p += n * H * 4;
    w.part = reinterpret_cast<float*>(p);
    p += (int64_t)grid_of(n) * P * 4;
    w.bytes = p - static_cast<char*>(ws);
    return w;
}

// [64 rows][64] of a row-major global array -> S (stride AS); rows >= n read as zero.
__device__ __forceinline__ void load_act(float* S, const float* __restrict__ g, int64_t row0,
                                         int64_t n, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (t >> 4) + 16 * q, col = 4 * (t & 15);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + row < n) v = *reinterpret_cast<const float4*>(g + (row0 + row) * H + col);
        *reinterpret_cast<float2*>(&S[row * AS + col]) = make_float2(v.x, v.y);
        *reinterpret_cast<float2*>(&S[row * AS + col + 2]) = make_float2(v.z, v.w);
    }
}
// and back, live rows only
__device__ __forceinline__ void store_act(const float* S, float* __restrict__ g, int64_t row0,
                                          int64_t n, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (t >> 4) + 16 * q, col = 4 * (t & 15);
        if (row0 + row >= n) continue;
        const float2 a = *reinterpret_cast<const float2*>(&S[row * AS + col]);
        const float2 b = *reinterpret_cast<const float2*>(&S[row * AS + col + 2]);
        *reinterpret_cast<float4*>(g + (row0 + row) * H + col) = make_float4(a.x, a.y, b.x, b.y);
    }
}

// PREP: (X, W1, W2) -> h1, h2.  Else: one product F v into this workgroup's partial.
template <bool PREP>
__global__ __launch_bounds__(TPB, 1) void fvp_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t n, int D, int A, Net net,
    const float* __restrict__ v, const double* __restrict__ cg_state, float* __restrict__ h1g,
    float* __restrict__ h2g, float* __restrict__ dz1g, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[L_END];
    if (!PREP && cg_state && cg_state[1] != 0.0) return;  // the solve has stopped
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int fi = w >> 1, ri = w & 1;
    float *W2S = sm + L_W2, *V2S = sm + L_V2, *W3S = sm + L_W3, *V3S = sm + L_V3;
    float *H1 = sm + L_H1, *H2 = sm + L_H2, *TA = sm + L_TA, *TB = sm + L_TB, *G = sm + L_G;
    float *VC = sm + L_TB, *XC = sm + L_XC, *vec = sm + L_VEC;
    const int64_t tiles = (n + TR - 1) / TR;
    const float* A1 = PREP ? net.w1 : v + net.off_w1;  // the first product's weight operand

    // per-workgroup constants: W2 (and the tangent's V2, W3, V3, biases) into LDS
    for (int i = t; i < H * H; i += TPB) {
        const int f = i >> 6, k = i & 63;
        W2S[f * AS + k] = net.w2[i];
        if (!PREP) V2S[f * AS + k] = v[net.off_w2 + i];
    }
    if (!PREP) {
        for (int i = t; i < AMAX * H; i += TPB) {
            const int a = i >> 6, k = i & 63;
            W3S[a * AS + k] = a < A ? net.w3[i] : 0.f;
            V3S[a * AS + k] = a < A ? v[net.off_w3 + i] : 0.f;
        }
    }
    if (t < H) {
        vec[V_C1 + t] = PREP ? net.b1[t] : v[net.off_b1 + t];
        vec[V_C2 + t] = PREP ? net.b2[t] : v[net.off_b2 + t];
    } else if (t < H + AMAX && !PREP) {
        const int a = t - H;
        vec[V_C3 + a] = a < A ? v[net.off_b3 + a] : 0.f;
        vec[V_IV + a] = a < A ? (float)(exp(-2.0 * (double)net.log_std[a]) / (double)n) : 0.f;
    }

    // chunk staging: thread t moves columns 4 (t & 7) .. + 3 of lines (t >> 3) + 32 q
    const int sc = 4 * (t & 7), sr = t >> 3;
    float4 xr[2], ar[2];
    const int nchunks = (D + KC - 1) / KC;

    f32x16 gW2 = zero16(), gW3 = zero16();
    // db2 (t < 64), db1 (t < 128), db3 (t < 160): one lane adds a whole column, so in f64 (a
    // sequential f32 sum of 64 rows was 3-4 x torch's error on the bias blocks)
    double gb = 0.0;

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        auto load = [&](int kc) {
            const int k = kc * KC + sc;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int line = sr + 32 * q;
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row0 + line < n && k < D) {  // D <= pitch and the pitch is 4-aligned
                    x = *reinterpret_cast<const float4*>(X + (row0 + line) * ldx + k);
                    if (k + 1 >= D) x.y = 0.f;
                    if (k + 2 >= D) x.z = 0.f;
                    if (k + 3 >= D) x.w = 0.f;
                }
                xr[q] = x;
                const float* a = A1 + (int64_t)line * D + k;  // flat vectors: 4-byte aligned only
                ar[q] = make_float4(k < D ? a[0] : 0.f, k + 1 < D ? a[1] : 0.f,
                                    k + 2 < D ? a[2] : 0.f, k + 3 < D ? a[3] : 0.f);
            }
        };
        auto store = [&](int buf) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                float* xd = &XC[(buf * TR + sr + 32 * q) * CS + sc];
                float* ad = &VC[(buf * H + sr + 32 * q) * CS + sc];
                *reinterpret_cast<float2*>(xd) = make_float2(xr[q].x, xr[q].y);
                *reinterpret_cast<float2*>(xd + 2) = make_float2(xr[q].z, xr[q].w);
                *reinterpret_cast<float2*>(ad) = make_float2(ar[q].x, ar[q].y);
                *reinterpret_cast<float2*>(ad + 2) = make_float2(ar[q].z, ar[q].w);
            }
        };
        load(0);
        if (!PREP) {
            load_act(H1, h1g, row0, n, t);
            load_act(H2, h2g, row0, n, t);
        }
        store(0);
        __syncthreads();
        // 1. Rz1^T (PREP: z1^T) [f][row] = sum_k V1[f][k] X[row][k]
        f32x16 acc = zero16();
        for (int kc = 0; kc < nchunks; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nchunks) load(kc + 1);
            gemm32(acc, KC, h, rowm(VC + buf * H * CS, CS, 32 * fi + c),
                   rowm(XC + buf * TR * CS, CS, 32 * ri + c));
            if (kc + 1 < nchunks) store(buf ^ 1);
            __syncthreads();
        }
        put_tile(TA, AS, acc, fi, ri, c, h, [&](float a, int row, int f) {
            const float z = a + vec[V_C1 + f];
            if (PREP) return tanhf(z);
            const float hh = H1[row * AS + f];
            return (1.0f - hh * hh) * z;
        });
        __syncthreads();
        // 2. Rz2^T = W2 Rh1^T + V2 h1^T (PREP: z2^T = W2 h1^T)
        acc = zero16();
        gemm32(acc, H, h, rowm(W2S, AS, 32 * fi + c), rowm(TA, AS, 32 * ri + c));
        if (!PREP) gemm32(acc, H, h, rowm(V2S, AS, 32 * fi + c), rowm(H1, AS, 32 * ri + c));
        put_tile(TB, AS, acc, fi, ri, c, h, [&](float a, int row, int f) {
            const float z = a + vec[V_C2 + f];
            if (PREP) return tanhf(z);
            const float hh = H2[row * AS + f];
            return (1.0f - hh * hh) * z;
        });
        __syncthreads();
        if (PREP) {
            store_act(TA, h1g, row0, n, t);
            store_act(TB, h2g, row0, n, t);
            __syncthreads();
            continue;
        }
        // 3. g^T [a][row] = (W3 Rh2^T + V3 h2^T + c3) exp(-2 log_std) / n; dead rows 0
        if (w < 2) {
            acc = zero16();
            gemm32(acc, H, h, rowm(W3S, AS, c), rowm(TB, AS, 32 * w + c));
            gemm32(acc, H, h, rowm(V3S, AS, c), rowm(H2, AS, 32 * w + c));
            put_tile(G, GS, acc, 0, w, c, h, [&](float a, int row, int f) {
                return row0 + row < n ? (a + vec[V_C3 + f]) * vec[V_IV + f] : 0.f;
            });
        }
        __syncthreads();
        // 4. dz2^T [f][row] = (sum_a W3[a][f] g[row][a]) (1 - h2^2)
        acc = zero16();
        gemm32(acc, AMAX, h, colm(W3S, AS, 32 * fi + c), rowm(G, GS, 32 * ri + c));
        put_tile(TB, AS, acc, fi, ri, c, h, [&](float a, int row, int f) {
            const float hh = H2[row * AS + f];
            return a * (1.0f - hh * hh);
        });
        __syncthreads();
        // 5. dz1^T [f][row] = (sum_f2 W2[f2][f] dz2[row][f2]) (1 - h1^2)
        acc = zero16();
        gemm32(acc, H, h, colm(W2S, AS, 32 * fi + c), rowm(TB, AS, 32 * ri + c));
        put_tile(TA, AS, acc, fi, ri, c, h, [&](float a, int row, int f) {
            const float hh = H1[row * AS + f];
            return a * (1.0f - hh * hh);
        });
        __syncthreads();
        // 6. weight gradients of layers 2-3 (k = row), bias gradients, dz1 for phase 2
        gemm32(gW2, TR, h, colm(TB, AS, 32 * fi + c), colm(H1, AS, 32 * ri + c));
        if (w >= 2) gemm32(gW3, TR, h, colm(G, GS, c), colm(H2, AS, 32 * (w - 2) + c));
        if (t < 2 * H + AMAX) {
            const float* S = t < H ? TB + t : t < 2 * H ? TA + (t - H) : G + (t - 2 * H);
            const int st = t < 2 * H ? AS : GS;
            double s = 0.0;
            for (int r = 0; r < TR; ++r) s += (double)S[r * st];
            gb += s;
        }
        store_act(TA, dz1g, row0, n, t);
        __syncthreads();
    }
    if (PREP) return;

    float* my = part + (int64_t)blockIdx.x * net.n_params;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = rho(r) + 4 * h;
        my[net.off_w2 + (32 * fi + i) * H + 32 * ri + c] = gW2[r];
        if (w >= 2 && i < A) my[net.off_w3 + i * H + 32 * (w - 2) + c] = gW3[r];
    }
    if (t < H) my[net.off_b2 + t] = (float)gb;
    else if (t < 2 * H) my[net.off_b1 + t - H] = (float)gb;
    else if (t < 2 * H + A) my[net.off_b3 + t - 2 * H] = (float)gb;

    // Phase 2: dW1 [f][k] = sum_row dz1[row][f] X[row][k], a panel of PANEL columns at a time.
    // Wave w: features 32 (w & 1) .., column tiles (w >> 1) + 2 i.  The accumulators stay in
    // registers across this workgroup's tiles.
    float *XS = sm + L_XS, *DZ = sm + L_DZ;
    const int ft = w & 1, kt0 = w >> 1;
    for (int p0 = 0; p0 < D; p0 += PANEL) {
        const int pc = D - p0 < PANEL ? D - p0 : PANEL;  // live columns of the panel
        const int pc4 = (pc + 3) >> 2, nkt = (pc + 31) >> 5;
        f32x16 g1[NKT];
#pragma unroll
        for (int i = 0; i < NKT; ++i) g1[i] = zero16();
        for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const int64_t row0 = tile * TR;
            __syncthreads();  // the previous tile's (and phase 1's) LDS reads
            for (int i = t; i < TR * pc4; i += TPB) {
                const int row = i / pc4, k = 4 * (i - row * pc4);
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row0 + row < n)
                    x = *reinterpret_cast<const float4*>(X + (row0 + row) * ldx + p0 + k);
                *reinterpret_cast<float2*>(&XS[row * XSTR + k]) = make_float2(x.x, x.y);
                *reinterpret_cast<float2*>(&XS[row * XSTR + k + 2]) = make_float2(x.z, x.w);
            }
            load_act(DZ, dz1g, row0, n, t);
            __syncthreads();
            const ColMajor fa = colm(DZ, AS, 32 * ft + c);
#pragma unroll 2
            for (int kk = 0; kk < TR; kk += 4) {
                const float2 a = fa(kk + 2 * h);
#pragma unroll
                for (int i = 0; i < NKT; ++i) {
                    const int kt = kt0 + 2 * i;
                    if (kt < nkt) {
                        const float2 b = colm(XS, XSTR, 32 * kt + c)(kk + 2 * h);
                        g1[i] = mfma(a.x, b.x, g1[i]);
                        g1[i] = mfma(a.y, b.y, g1[i]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int k = 32 * (kt0 + 2 * i) + c;
            if (k >= pc) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                my[net.off_w1 + (int64_t)(32 * ft + rho(r) + 4 * h) * D + p0 + k] = g1[i][r];
        }
    }
}

// out = sum of the partials (workgroup order) + damping v; the log-std block is 2 v + damping v.
// pz[block] = sum over the block's elements of v[j] out[j], f64.
__global__ __launch_bounds__(TPB) void fvp_fold_kernel(
    const float* __restrict__ part, int nparts, int64_t P, int64_t off_sigma, int A,
    const float* __restrict__ v, float damping, const double* __restrict__ cg_state,
    float* __restrict__ out, double* __restrict__ pz) {
#pragma clang fp contract(off)
    __shared__ double sh[TPB / kWave];
    if (cg_state && cg_state[1] != 0.0) return;
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    double d = 0.0;
    if (j < P) {
        const float vj = v[j];
        float s;
        if (j >= off_sigma && j < off_sigma + A) {
            s = 2.0f * vj;
        } else {
            double acc = 0.0;
            for (int g = 0; g < nparts; ++g) acc += (double)part[(int64_t)g * P + j];
            s = (float)acc;
        }
        const float o = s + damping * vj;
        out[j] = o;
        d = (double)vj * (double)o;
    }
    d = block_sum(d, sh);
    if (threadIdx.x == 0) pz[blockIdx.x] = d;
}

constexpr int CG_TPB = 1024;

__global__ __launch_bounds__(CG_TPB) void cg_init_kernel(const float* __restrict__ b, int64_t P,
                                                         float* __restrict__ x,
                                                         float* __restrict__ r,
                                                         float* __restrict__ p,
                                                         double* __restrict__ state) {
    __shared__ double sh[CG_TPB / kWave];
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < P; j += CG_TPB) {
        const float bj = b[j];
        x[j] = 0.f;
        r[j] = bj;
        p[j] = bj;
        s += (double)bj * (double)bj;
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) {
        state[0] = s;    // r.r
        state[1] = 0.0;  // stopped
    }
}

// npg.py:151-160 after z = MVP(p): alpha = rdotr / p.z, x += alpha p, r -= alpha z, the stop
// test, p = r + new_rdotr / rdotr p.  x already holds the stopping iteration's alpha p.
__global__ __launch_bounds__(CG_TPB) void cg_step_kernel(float* __restrict__ x,
                                                         float* __restrict__ r,
                                                         float* __restrict__ p,
                                                         const float* __restrict__ z, int64_t P,
                                                         double tol, double* __restrict__ state,
                                                         const double* __restrict__ pz, int npz) {
    __shared__ double sh[CG_TPB / kWave];
    const double rdotr = state[0];
    if (state[1] != 0.0) return;
    double s = 0.0;
    for (int i = threadIdx.x; i < npz; i += CG_TPB) s += pz[i];
    const double alpha = rdotr / block_sum(s, sh);
    s = 0.0;
    for (int64_t j = threadIdx.x; j < P; j += CG_TPB) {
        x[j] = (float)((double)x[j] + alpha * (double)p[j]);
        const float rj = (float)((double)r[j] - alpha * (double)z[j]);
        r[j] = rj;
        s += (double)rj * (double)rj;
    }
    const double new_rdotr = block_sum(s, sh);  // its barriers also order the state reads above
    if (new_rdotr < tol) {                      // false for NaN, as in the reference
        if (threadIdx.x == 0) state[1] = 1.0;
        return;
    }
    const double beta = new_rdotr / rdotr;
    for (int64_t j = threadIdx.x; j < P; j += CG_TPB)
        p[j] = (float)((double)r[j] + beta * (double)p[j]);
    if (threadIdx.x == 0) state[0] = new_rdotr;
}

int check_shape(const char* what, const float* X, int64_t ldx, int64_t n, int64_t D, int64_t A,
                const tsrl_fvp_net* net, const void* ws, int64_t ws_bytes) {
    TSRL_CHECK_ARG(n >= 1 && n < ((int64_t)1 << 31), "%s: need 1 <= n < 2^31 (got %lld)", what,
                   (long long)n);
    TSRL_CHECK_ARG(D >= 1 && D < (1 << 20), "%s: need 1 <= D < 2^20 (got %lld)", what,
                   (long long)D);
    TSRL_CHECK_ARG(A >= 1 && A <= AMAX, "%s: need 1 <= A <= %d (got %lld)", what, AMAX,
                   (long long)A);
    TSRL_CHECK_ARG(X && net && ws, "%s: null pointer", what);
    TSRL_CHECK_ARG(ldx % 4 == 0 && ldx >= (D + 3) / 4 * 4 && aligned16(X),
                   "%s: rows must be 16-byte aligned and roundup(D, 4) floats apart at least "
                   "(pitch %lld, D %lld)", what, (long long)ldx, (long long)D);
    TSRL_CHECK_ARG(net->w1 && net->b1 && net->w2 && net->b2 && net->w3 && net->b3 && net->log_std,
                   "%s: null weight pointer", what);
    TSRL_CHECK_ARG(net->n_params == n_params_of(D, A), "%s: n_params %lld, the actor has %lld",
                   what, (long long)net->n_params, (long long)n_params_of(D, A));
    const int64_t offs[7] = {net->off_sigma, net->off_w1, net->off_b1, net->off_w2,
                             net->off_b2,    net->off_w3, net->off_b3};
    const int64_t lens[7] = {A, H * D, H, H * H, H, A * H, A};
    for (int i = 0; i < 7; ++i)
        TSRL_CHECK_ARG(offs[i] >= 0 && offs[i] + lens[i] <= net->n_params,
                       "%s: parameter block %d lies outside the flat vector", what, i);
    TSRL_CHECK_ARG(aligned16(ws) && ws_bytes >= tsrl_fvp_workspace_bytes(n, D, A),
                   "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", what,
                   (long long)tsrl_fvp_workspace_bytes(n, D, A), (long long)ws_bytes);
    return 0;
}

Net net_of(const tsrl_fvp_net* s) {
    return Net{s->w1,     s->b1,      s->w2,     s->b2,     s->w3,     s->b3,     s->log_std,
               s->off_sigma, s->off_w1, s->off_b1, s->off_w2, s->off_b2, s->off_w3, s->off_b3,
               s->n_params};
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int64_t tsrl_fvp_workspace_bytes(int64_t n, int64_t D, int64_t A) {
    if (n < 1 || D < 1 || A < 1 || A > AMAX) return 0;
    return carve(nullptr, n, D, A).bytes;
}

extern "C" int tsrl_fvp_prepare(const float* X, int64_t ldx, int64_t n, int64_t D, int64_t A,
                                const tsrl_fvp_net* net, void* ws, int64_t ws_bytes,
                                void* stream) {
    if (int rc = check_shape("tsrl_fvp_prepare", X, ldx, n, D, A, net, ws, ws_bytes)) return rc;
    const Ws w = carve(ws, n, D, A);
    hipLaunchKernelGGL(fvp_kernel<true>, dim3(grid_of(n)), dim3(TPB), 0, as_stream(stream), X,
                       ldx, n, (int)D, (int)A, net_of(net), (const float*)nullptr,
                       (const double*)nullptr, w.h1, w.h2, w.dz1, w.part);
    TSRL_LAUNCH_CHECK("tsrl_fvp_prepare");
    return 0;
}

extern "C" int tsrl_fvp_apply(const float* X, int64_t ldx, int64_t n, int64_t D, int64_t A,
                              const tsrl_fvp_net* net, const float* v, float* out,
                              double damping, const double* cg_state, void* ws,
                              int64_t ws_bytes, void* stream) {
    if (int rc = check_shape("tsrl_fvp_apply", X, ldx, n, D, A, net, ws, ws_bytes)) return rc;
    TSRL_CHECK_ARG(v && out && v != out, "tsrl_fvp_apply: v and out must be two vectors");
    const Ws w = carve(ws, n, D, A);
    const int grid = grid_of(n);
    const int64_t P = net->n_params;
    hipLaunchKernelGGL(fvp_kernel<false>, dim3(grid), dim3(TPB), 0, as_stream(stream), X, ldx, n,
                       (int)D, (int)A, net_of(net), v, cg_state, w.h1, w.h2, w.dz1, w.part);
    TSRL_LAUNCH_CHECK("tsrl_fvp_apply");
    hipLaunchKernelGGL(fvp_fold_kernel, dim3((unsigned)fold_blocks(P)), dim3(TPB), 0,
                       as_stream(stream), w.part, grid, P, net->off_sigma, (int)A, v,
                       (float)damping, cg_state, out, w.pz);
    TSRL_LAUNCH_CHECK("tsrl_fvp_apply (fold)");
    return 0;
}

extern "C" int tsrl_cg_init(const float* b, int64_t P, float* x, float* r, float* p,
                            double* state, void* stream) {
    TSRL_CHECK_ARG(P >= 1, "tsrl_cg_init: need P >= 1");
    TSRL_CHECK_ARG(b && x && r && p && state, "tsrl_cg_init: null pointer");
    hipLaunchKernelGGL(cg_init_kernel, dim3(1), dim3(CG_TPB), 0, as_stream(stream), b, P, x, r, p,
                       state);
    TSRL_LAUNCH_CHECK("tsrl_cg_init");
    return 0;
}

extern "C" int tsrl_cg_step(float* x, float* r, float* p, const float* z, int64_t P,
                            double residual_tol, double* state, const void* fvp_ws,
                            void* stream) {
    TSRL_CHECK_ARG(P >= 1, "tsrl_cg_step: need P >= 1");
    TSRL_CHECK_ARG(x && r && p && z && state && fvp_ws, "tsrl_cg_step: null pointer");
    hipLaunchKernelGGL(cg_step_kernel, dim3(1), dim3(CG_TPB), 0, as_stream(stream), x, r, p, z, P,
                       residual_tol, state, static_cast<const double*>(fvp_ws),
                       (int)fold_blocks(P));
    TSRL_LAUNCH_CHECK("tsrl_cg_step");
    return 0;
}
