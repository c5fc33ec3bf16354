// The discriminator of GAILPolicy (tianshou/policy/imitation/gail.py, examples/inverse/
// irl_gail.py): Linear(D + A, 64)-Tanh-Linear(64, 64)-Tanh-Linear(64, 1) over rows whose first D
// columns live in an observation array and whose last A columns live in an action array, each
// read through its own pitch and (optional) int64 row index.  No concatenated row and no gathered
// copy of a row is written to memory.  Kernels:
//   gail_reward_kernel  forward only: rew[r] = softplus(d[r]).  Layer 1 streams 32-column chunks
//                       of X and W1 through a two-deep LDS ring; the chunk loop runs over the
//                       logical columns 0 .. D + A, so a chunk may take columns from both arrays.
//                       W2, w3 and the biases stay in LDS over the tiles a workgroup walks; h2 and
//                       d are formed from the layer-2 accumulators in registers.  71 KB of LDS:
//                       two workgroups per CU.
//   gail_step_kernel    one discriminator step: per 64-row tile the X panel (up to 384 columns) is
//                       staged into LDS once and serves layer 1 (read by rows) and dW1 = dz1^T X
//                       (read by columns); forward, loss terms, backward chain and the six
//                       gradients follow in the same tile visit.  One partial per workgroup.
//   gail_fold_kernel    sums the partials in workgroup order, writes loss / acc_pi / acc_exp.
//
// Every product is v_mfma_f32_32x32x2f32 on f32 operands with fvp.hip's conventions: 4 waves, a
// 64 x 64 result is four 32 x 32 tiles (wave w: features 32 (w >> 1), rows 32 (w & 1)); lane
// (c = l & 31, h = l >> 5) supplies A[i = c][k] and B[k][j = c] for k = kk + 2h, kk + 2h + 1;
// activations are row-major [row][feature] with stride 66, the X panel has stride 386 (both 2 mod
// 32: 8-byte row reads and column reads are conflict-free); C register r of lane (c, h) is
// element [rho(r) + 4h][c].
//
// The step kernel's LDS does not hold the panel, W2, h1, h2, dz1, dz2 and a W1 chunk ring at once
// (183 KB).  dz2 overwrites h2 (after dW3 has read it) and dz1 overwrites h1 (after dW2 has read
// it); W1 is re-read from L2 per tile through ONE 64 x 32 chunk buffer, the next chunk held in
// registers while the current one feeds the MFMAs.  D + A > 384: the forward accumulates over the
// panels in turn, the last panel stays for its dW1 columns, dz1 goes to the workspace and a
// second pass per earlier panel re-stages it (fvp.hip's phase 2).
//
// Pad rows of a last tile read the last live row of their kind (a clamped row number), so every
// activation of a pad row is as finite as a live row's; they enter the gradients through g = 0 and
// the sums not at all.  No atomics: two calls on the same inputs are bitwise equal.
#include "tsrl_common.h"

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int H = 64;            // hidden width
constexpr int TR = 64;           // rows of a tile
constexpr int TPB = 256;         // 4 waves
constexpr int AS = 66;           // stride of a [64][64] activation / weight array in LDS
constexpr int KC = 32;           // K chunk of the first layer
constexpr int CS = 34;           // stride of a staged chunk [64][32]
constexpr int PANEL = 384;       // X columns resident in the step kernel
constexpr int XSTR = PANEL + 2;  // their LDS stride (2 mod 32, as CS)
constexpr int NKT = PANEL / 32 / 2;  // dW1 column tiles per wave
constexpr int NVEC = 3 * H + 4;  // b1, b2, w3, b3

// LDS map of the reward kernel (floats)
constexpr int R_W2 = 0, R_H1 = R_W2 + H * AS, R_WC = R_H1 + TR * AS, R_XC = R_WC + 2 * H * CS,
              R_VEC = R_XC + 2 * TR * CS, R_PD = R_VEC + NVEC, R_END = R_PD + 2 * TR;
static_assert(2 * R_END * 4 <= 163840, "gail reward: two workgroups per CU");
// LDS map of the step kernel (floats); RO holds 2 x 64 int64 row offsets
constexpr int S_XS = 0, S_W2 = S_XS + TR * XSTR, S_H1 = S_W2 + H * AS, S_H2 = S_H1 + TR * AS,
              S_WC = S_H2 + TR * AS, S_VEC = S_WC + H * CS, S_G = S_VEC + NVEC, S_PD = S_G + TR,
              S_RO = S_PD + 2 * TR, S_END = S_RO + 4 * TR;
static_assert(S_END * 4 <= 163840, "gail step LDS");
static_assert(S_RO % 2 == 0, "int64 row offsets need 8-byte alignment");
static_assert(XSTR % 2 == 0 && AS % 2 == 0 && CS % 2 == 0, "float2 operand reads");

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

// C tile (it, jt) -> S[32 jt + c][32 it + rho(r) + 4h] = f(acc, row, feature)
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

// The two arrays of one kind of row.  ov / av: 16-byte loads are safe from obs / act (base and
// pitch 16-byte aligned; for act also D % 4 == 0, so that a 4-column group starts on a float4).
struct Rows {
    const float* obs;
    int64_t ldo;
    const int64_t* io;
    const float* act;
    int64_t lda;
    const int64_t* ia;
    int ov, av;
};
struct Net {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
};
// field by field: a reference to one of two kernel arguments would keep both in memory
__device__ __forceinline__ Rows pick(bool second, const Rows& a, const Rows& b) {
    return Rows{second ? b.obs : a.obs, second ? b.ldo : a.ldo, second ? b.io : a.io,
                second ? b.act : a.act, second ? b.lda : a.lda, second ? b.ia : a.ia,
                second ? b.ov : a.ov,   second ? b.av : a.av};
}

// Logical columns k .. k + 3 (k % 4 == 0) of the row at float offsets (ro, ra) of obs / act:
// columns < D from obs, < K = D + A from act, zero beyond.  A group inside one array is one
// 16-byte load where that array allows it; a group across the boundary, or in an array that does
// not, is four scalar loads.
__device__ __forceinline__ float4 load4(const Rows& R, int64_t ro, int64_t ra, int k, int D,
                                        int K) {
    if (k + 3 < D && R.ov) return *reinterpret_cast<const float4*>(R.obs + ro + k);
    if (k >= D && k + 3 < K && R.av) return *reinterpret_cast<const float4*>(R.act + ra + (k - D));
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int kk = k + j;
        v[j] = kk < D ? R.obs[ro + kk] : kk < K ? R.act[ra + (kk - D)] : 0.f;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// W1[line][k .. k + 3] of the [64, K] weight (4-byte aligned only), zero beyond K
__device__ __forceinline__ float4 load_w4(const float* __restrict__ w1, int line, int k, int K) {
    const float* a = w1 + (int64_t)line * K + k;
    return make_float4(k < K ? a[0] : 0.f, k + 1 < K ? a[1] : 0.f, k + 2 < K ? a[2] : 0.f,
                       k + 3 < K ? a[3] : 0.f);
}

__device__ __forceinline__ void put4(float* d, float4 v) {
    *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
}

// W2 [f][k] at stride AS; b1, b2, w3, b3 into vec
__device__ __forceinline__ void load_consts(float* W2S, float* vec, const Net& net, int t) {
    for (int i = t; i < H * H; i += TPB) W2S[(i >> 6) * AS + (i & 63)] = net.w2[i];
    if (t < H) {
        vec[t] = net.b1[t];
        vec[H + t] = net.b2[t];
        vec[2 * H + t] = net.w3[t];
    }
    if (t == 0) vec[3 * H] = net.b3[0];
}

// softplus(s) and sigmoid(s) from one exp(-|s|)
__device__ __forceinline__ float softplus_sig(float s, float* sig) {
    const float e = expf(-fabsf(s));
    *sig = (s >= 0.f ? 1.0f : e) / (1.0f + e);
    return fmaxf(s, 0.f) + log1pf(e);
}

__global__ __launch_bounds__(TPB, 2) void gail_reward_kernel(Rows R, int64_t n, int D, int A,
                                                             Net net, float* __restrict__ rew) {
    __shared__ __attribute__((aligned(16))) float sm[R_END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int fi = w >> 1, ri = w & 1;
    float *W2S = sm + R_W2, *H1 = sm + R_H1, *WC = sm + R_WC, *XC = sm + R_XC;
    float *vec = sm + R_VEC, *PD = sm + R_PD;
    const int K = D + A, nchunks = (K + KC - 1) / KC;
    const int64_t tiles = (n + TR - 1) / TR;
    load_consts(W2S, vec, net, t);

    // chunk staging: thread t moves columns 4 (t & 7) .. + 3 of lines (t >> 3) + 32 q
    const int sc = 4 * (t & 7), sr = t >> 3;
    float4 xr[2], ar[2];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        int64_t ro[2], ra[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // rows past n read row n - 1 and are never stored
            int64_t r = row0 + sr + 32 * q;
            r = r < n ? r : n - 1;
            ro[q] = (R.io ? R.io[r] : r) * R.ldo;
            ra[q] = (R.ia ? R.ia[r] : r) * R.lda;
        }
        auto load = [&](int kc) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                xr[q] = load4(R, ro[q], ra[q], kc * KC + sc, D, K);
                ar[q] = load_w4(net.w1, sr + 32 * q, kc * KC + sc, K);
            }
        };
        auto store = [&](int buf) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                put4(&XC[(buf * TR + sr + 32 * q) * CS + sc], xr[q]);
                put4(&WC[(buf * H + sr + 32 * q) * CS + sc], ar[q]);
            }
        };
        load(0);
        store(0);
        __syncthreads();
        // z1^T [f][row] = sum_k W1[f][k] X[row][k], k over both arrays
        f32x16 acc = zero16();
        for (int kc = 0; kc < nchunks; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < nchunks) load(kc + 1);
            gemm32(acc, KC, h, rowm(WC + buf * H * CS, CS, 32 * fi + c),
                   rowm(XC + buf * TR * CS, CS, 32 * ri + c));
            if (kc + 1 < nchunks) store(buf ^ 1);
            __syncthreads();
        }
        put_tile(H1, AS, acc, fi, ri, c, h,
                 [&](float a, int, int f) { return tanhf(a + vec[f]); });
        __syncthreads();
        // z2^T = W2 h1^T; the lane holds 16 features of row 32 ri + c: its share of w3 . h2
        acc = zero16();
        gemm32(acc, H, h, rowm(W2S, AS, 32 * fi + c), rowm(H1, AS, 32 * ri + c));
        float pd = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = 32 * fi + rho(r) + 4 * h;
            pd += vec[2 * H + f] * tanhf(acc[r] + vec[H + f]);
        }
        pd += __shfl_xor(pd, 32, kWave);
        if (h == 0) PD[fi * TR + 32 * ri + c] = pd;
        __syncthreads();
        if (t < TR && row0 + t < n) {
            float sig;
            rew[row0 + t] = softplus_sig(PD[t] + PD[TR + t] + vec[3 * H], &sig);
        }
    }
}

// [64 rows][64] of a row-major global array <-> S (stride AS)
__device__ __forceinline__ void load_act(float* S, const float* __restrict__ g, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (t >> 4) + 16 * q, col = 4 * (t & 15);
        put4(&S[row * AS + col], *reinterpret_cast<const float4*>(g + row * H + col));
    }
}
__device__ __forceinline__ void store_act(const float* S, float* __restrict__ g, int t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (t >> 4) + 16 * q, col = 4 * (t & 15);
        const float2 a = *reinterpret_cast<const float2*>(&S[row * AS + col]);
        const float2 b = *reinterpret_cast<const float2*>(&S[row * AS + col + 2]);
        *reinterpret_cast<float4*>(g + row * H + col) = make_float4(a.x, a.y, b.x, b.y);
    }
}

// Flat gradient layout: disc_net.parameters() order
__host__ __device__ inline int64_t n_params_of(int64_t K) { return H * K + H + H * H + H + H + 1; }

// Tiles 0 .. tiles_pi - 1 hold policy rows, the rest expert rows.
__global__ __launch_bounds__(TPB, 1) void gail_step_kernel(Rows Rp, Rows Re, int64_t m_pi,
                                                           int64_t m_exp, int D, int A, Net net,
                                                           float* __restrict__ part,
                                                           double* __restrict__ sums,
                                                           float* __restrict__ dz1g) {
    __shared__ __attribute__((aligned(16))) float sm[S_END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int fi = w >> 1, ri = w & 1;
    float *XS = sm + S_XS, *W2S = sm + S_W2, *H1 = sm + S_H1, *H2 = sm + S_H2, *WC = sm + S_WC;
    float *vec = sm + S_VEC, *G = sm + S_G, *PD = sm + S_PD;
    int64_t* RO = reinterpret_cast<int64_t*>(sm + S_RO);
    int64_t* RA = RO + TR;
    const int K = D + A;
    const int p_last = (K - 1) / PANEL * PANEL;  // the panel that stays for its dW1 columns
    const int64_t tiles_pi = (m_pi + TR - 1) / TR;
    const int64_t tiles = tiles_pi + (m_exp + TR - 1) / TR;
    load_consts(W2S, vec, net, t);

    const int sc = 4 * (t & 7), sr = t >> 3;  // W1 chunk staging, as in the reward kernel
    const int ft = w & 1, kt0 = w >> 1;       // dW1: features 32 ft .., column tiles kt0 + 2 i
    f32x16 gW2 = zero16(), g1[NKT];
#pragma unroll
    for (int i = 0; i < NKT; ++i) g1[i] = zero16();
    // wave 0: lane = row: loss sums, counts, sum g (db3); then lane = feature: dW3.
    // wave 1: db2, wave 2: db1 (lane = feature).  One lane adds a whole column, so in f64.
    double s_pi = 0.0, s_exp = 0.0, c_pi = 0.0, c_exp = 0.0, sg = 0.0, gcol = 0.0;

    // row offsets of the tile's 64 rows (pad rows: the last live row of the kind)
    auto row_offsets = [&](const Rows& R, int64_t base, int64_t m) {
        if (t < TR) {
            int64_t r = base + t;
            r = r < m ? r : m - 1;
            RO[t] = (R.io ? R.io[r] : r) * R.ldo;
            RA[t] = (R.ia ? R.ia[r] : r) * R.lda;
        }
    };
    // columns p0 .. p0 + roundup(pc, 32) of the tile's rows -> XS (zero beyond K)
    auto stage = [&](const Rows& R, int p0, int pc) {
        const int pc4 = (pc + 31) / 32 * 8;
        for (int i = t; i < TR * pc4; i += TPB) {
            const int row = i / pc4, k = 4 * (i - row * pc4);
            put4(&XS[row * XSTR + k], load4(R, RO[row], RA[row], p0 + k, D, K));
        }
    };
    // dW1 columns of the panel in XS: g1 += dz1^T X, dz1 in H1
    auto dw1 = [&](int pc) {
        const int nkt = (pc + 31) >> 5;
        const ColMajor fa = colm(H1, AS, 32 * ft + c);
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
    };
    float* my = part + (int64_t)blockIdx.x * n_params_of(K);
    const int64_t off_b1 = (int64_t)H * K, off_w2 = off_b1 + H, off_b2 = off_w2 + H * H,
                  off_w3 = off_b2 + H, off_b3 = off_w3 + H;
    auto write_dw1 = [&](int p0, int pc) {
#pragma unroll
        for (int i = 0; i < NKT; ++i) {
            const int k = 32 * (kt0 + 2 * i) + c;
            if (k >= pc) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                my[(int64_t)(32 * ft + rho(r) + 4 * h) * K + p0 + k] = g1[i][r];
        }
    };

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const bool expert = tile >= tiles_pi;
        const Rows R = pick(expert, Rp, Re);
        const int64_t base = (expert ? tile - tiles_pi : tile) * TR;
        const int64_t m = expert ? m_exp : m_pi;
        __syncthreads();  // the previous tile's reads of XS, H1, RO
        row_offsets(R, base, m);
        __syncthreads();
        // 1. z1^T [f][row] = sum_k W1[f][k] X[row][k] over the panels; W1 by chunks through WC
        f32x16 acc = zero16();
        for (int p0 = 0; p0 < K; p0 += PANEL) {
            const int pc = K - p0 < PANEL ? K - p0 : PANEL;
            const int nch = (pc + KC - 1) / KC;
            float4 ar[2];
            stage(R, p0, pc);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                put4(&WC[(sr + 32 * q) * CS + sc], load_w4(net.w1, sr + 32 * q, p0 + sc, K));
            __syncthreads();
            for (int kc = 0; kc < nch; ++kc) {
                const bool more = kc + 1 < nch;
                if (more) {
#pragma unroll
                    for (int q = 0; q < 2; ++q)
                        ar[q] = load_w4(net.w1, sr + 32 * q, p0 + (kc + 1) * KC + sc, K);
                }
                gemm32(acc, KC, h, rowm(WC, CS, 32 * fi + c),
                       rowm(XS + kc * KC, XSTR, 32 * ri + c));
                __syncthreads();
                if (more) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) put4(&WC[(sr + 32 * q) * CS + sc], ar[q]);
                    __syncthreads();
                }
            }
        }
        put_tile(H1, AS, acc, fi, ri, c, h,
                 [&](float a, int, int f) { return tanhf(a + vec[f]); });
        __syncthreads();
        // 2. h2 and each lane's share of w3 . h2
        acc = zero16();
        gemm32(acc, H, h, rowm(W2S, AS, 32 * fi + c), rowm(H1, AS, 32 * ri + c));
        float pd = 0.f;
        put_tile(H2, AS, acc, fi, ri, c, h, [&](float a, int, int f) {
            const float hh = tanhf(a + vec[H + f]);
            pd += vec[2 * H + f] * hh;
            return hh;
        });
        pd += __shfl_xor(pd, 32, kWave);
        if (h == 0) PD[fi * TR + 32 * ri + c] = pd;
        __syncthreads();
        // 3. per row: d, the loss term, the count, g = dLoss/dd
        if (t < TR) {
            const float d = PD[t] + PD[TR + t] + vec[3 * H];
            const float s = expert ? -d : d;  // the loss is softplus(d_pi), softplus(-d_exp)
            float sig;
            const float sp = softplus_sig(s, &sig);
            float g = 0.f;
            if (base + t < m) {
                g = (float)((double)(expert ? -sig : sig) / (double)m);
                if (expert) {
                    s_exp += (double)sp;
                    c_exp += s < 0.f ? 1.0 : 0.0;  // d_exp > 0
                } else {
                    s_pi += (double)sp;
                    c_pi += s < 0.f ? 1.0 : 0.0;  // d_pi < 0
                }
            }
            sg += (double)g;
            G[t] = g;
        }
        __syncthreads();
        // 4. dW3[f] = sum_row g h2
        if (t < H) {
            double a = 0.0;
            for (int r = 0; r < TR; ++r) a += (double)G[r] * (double)H2[r * AS + t];
            gcol += a;
        }
        __syncthreads();
        // 5. dz2 = g w3 (1 - h2^2) over h2
        for (int i = t; i < TR * H; i += TPB) {
            const int row = i >> 6, f = i & 63;
            const float hh = H2[row * AS + f];
            H2[row * AS + f] = G[row] * vec[2 * H + f] * (1.0f - hh * hh);
        }
        __syncthreads();
        // 6. dW2 += dz2^T h1; dz1^T [f][row] = sum_f2 W2[f2][f] dz2[row][f2]; db2
        gemm32(gW2, TR, h, colm(H2, AS, 32 * fi + c), colm(H1, AS, 32 * ri + c));
        acc = zero16();
        gemm32(acc, H, h, colm(W2S, AS, 32 * fi + c), rowm(H2, AS, 32 * ri + c));
        if (w == 1) {
            double a = 0.0;
            for (int r = 0; r < TR; ++r) a += (double)H2[r * AS + l];
            gcol += a;
        }
        __syncthreads();  // dW2 has read h1
        put_tile(H1, AS, acc, fi, ri, c, h, [&](float a, int row, int f) {
            const float hh = H1[row * AS + f];
            return a * (1.0f - hh * hh);
        });
        __syncthreads();
        // 7. db1, dW1 of the panel in XS; dz1 out for the earlier panels
        if (w == 2) {
            double a = 0.0;
            for (int r = 0; r < TR; ++r) a += (double)H1[r * AS + l];
            gcol += a;
        }
        dw1(K - p_last);
        if (p_last > 0) store_act(H1, dz1g + tile * TR * H, t);
    }
    write_dw1(p_last, K - p_last);
#pragma unroll
    for (int r = 0; r < 16; ++r)
        my[off_w2 + (32 * fi + rho(r) + 4 * h) * H + 32 * ri + c] = gW2[r];
    if (w == 0) {
        my[off_w3 + l] = (float)gcol;
        s_pi = wave_sum(s_pi);
        s_exp = wave_sum(s_exp);
        c_pi = wave_sum(c_pi);
        c_exp = wave_sum(c_exp);
        sg = wave_sum(sg);
        if (l == 0) {
            my[off_b3] = (float)sg;
            double* o = sums + 4 * (int64_t)blockIdx.x;
            o[0] = s_pi;
            o[1] = s_exp;
            o[2] = c_pi;
            o[3] = c_exp;
        }
    } else if (w == 1) {
        my[off_b2 + l] = (float)gcol;
    } else if (w == 2) {
        my[off_b1 + l] = (float)gcol;
    }

    // D + A > 384: dW1 of the earlier panels from the stored dz1
    for (int p0 = 0; p0 < p_last; p0 += PANEL) {
#pragma unroll
        for (int i = 0; i < NKT; ++i) g1[i] = zero16();
        for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            const bool expert = tile >= tiles_pi;
            const Rows R = pick(expert, Rp, Re);
            __syncthreads();
            row_offsets(R, (expert ? tile - tiles_pi : tile) * TR, expert ? m_exp : m_pi);
            __syncthreads();
            stage(R, p0, PANEL);
            load_act(H1, dz1g + tile * TR * H, t);
            __syncthreads();
            dw1(PANEL);
        }
        write_dw1(p0, PANEL);
    }
}

// grad = sum of the partials in workgroup order; out3 = loss, acc_pi, acc_exp
__global__ __launch_bounds__(TPB) void gail_fold_kernel(const float* __restrict__ part,
                                                        const double* __restrict__ sums,
                                                        int nparts, int64_t P, double m_pi,
                                                        double m_exp, float* __restrict__ grad,
                                                        float* __restrict__ out3) {
    const int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (j < P) {
        double acc = 0.0;
        for (int g = 0; g < nparts; ++g) acc += (double)part[(int64_t)g * P + j];
        grad[j] = (float)acc;
    }
    if (j == 0) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int g = 0; g < nparts; ++g)
            for (int i = 0; i < 4; ++i) s[i] += sums[4 * (int64_t)g + i];
        out3[0] = (float)(s[0] / m_pi + s[1] / m_exp);
        out3[1] = (float)(s[2] / m_pi);
        out3[2] = (float)(s[3] / m_exp);
    }
}

struct Ws {
    double* sums;
    float *part, *dz1;
    int64_t bytes;
};
inline int64_t tiles_of(int64_t m) { return (m + TR - 1) / TR; }
inline int step_grid(int64_t m_pi, int64_t m_exp) {
    const int64_t tiles = tiles_of(m_pi) + tiles_of(m_exp);
    return (int)(tiles < n_cus() ? tiles : n_cus());
}
inline Ws carve(void* ws, int64_t m_pi, int64_t m_exp, int64_t K) {
    const int64_t grid = step_grid(m_pi, m_exp);
    char* p = static_cast<char*>(ws);
    Ws w;
    w.sums = reinterpret_cast<double*>(p);
    p += grid * 4 * 8;
    w.part = reinterpret_cast<float*>(p);
    p += (grid * n_params_of(K) * 4 + 15) / 16 * 16;
    w.dz1 = reinterpret_cast<float*>(p);
    if (K > PANEL) p += (tiles_of(m_pi) + tiles_of(m_exp)) * TR * H * 4;
    w.bytes = p - static_cast<char*>(ws);
    return w;
}

bool dims_ok(int64_t D, int64_t A) { return D >= 1 && A >= 1 && D + A < (1 << 20); }

int check_dims(const char* what, int64_t D, int64_t A, const tsrl_gail_net* net) {
    TSRL_CHECK_ARG(dims_ok(D, A), "%s: need obs_dim >= 1, act_dim >= 1, obs_dim + act_dim < 2^20 "
                   "(got %lld, %lld)", what, (long long)D, (long long)A);
    TSRL_CHECK_ARG(net && net->w1 && net->b1 && net->w2 && net->b2 && net->w3 && net->b3,
                   "%s: null weight pointer", what);
    return 0;
}

int check_rows(const char* what, const char* kind, const tsrl_gail_rows* r, int64_t D, int64_t A) {
    TSRL_CHECK_ARG(r && r->obs && r->act, "%s: null %s rows", what, kind);
    TSRL_CHECK_ARG(r->ldo >= D && r->lda >= A,
                   "%s: %s row pitches (%lld, %lld floats) are shorter than the rows (%lld, %lld)",
                   what, kind, (long long)r->ldo, (long long)r->lda, (long long)D, (long long)A);
    TSRL_CHECK_ARG((reinterpret_cast<uintptr_t>(r->obs) & 3u) == 0 &&
                   (reinterpret_cast<uintptr_t>(r->act) & 3u) == 0,
                   "%s: %s rows must be 4-byte aligned", what, kind);
    return 0;
}

Rows rows_of(const tsrl_gail_rows* r, int64_t D) {
    return Rows{r->obs, r->ldo, r->io, r->act, r->lda, r->ia,
                r->ldo % 4 == 0 && aligned16(r->obs),
                r->lda % 4 == 0 && aligned16(r->act) && D % 4 == 0};
}

Net net_of(const tsrl_gail_net* s) { return Net{s->w1, s->b1, s->w2, s->b2, s->w3, s->b3}; }

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_gail_reward(const tsrl_gail_rows* rows, int64_t n, int64_t D, int64_t A,
                                const tsrl_gail_net* net, float* rew, void* stream) {
    TSRL_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "tsrl_gail_reward: need 0 <= n < 2^31 (got "
                   "%lld)", (long long)n);
    if (int rc = check_dims("tsrl_gail_reward", D, A, net)) return rc;
    if (int rc = check_rows("tsrl_gail_reward", "the", rows, D, A)) return rc;
    if (n == 0) return 0;
    TSRL_CHECK_ARG(rew, "tsrl_gail_reward: null output");
    const int64_t tiles = tiles_of(n), cap = 2 * (int64_t)n_cus();
    hipLaunchKernelGGL(gail_reward_kernel, dim3((unsigned)(tiles < cap ? tiles : cap)), dim3(TPB),
                       0, as_stream(stream), rows_of(rows, D), n, (int)D, (int)A, net_of(net),
                       rew);
    TSRL_LAUNCH_CHECK("tsrl_gail_reward");
    return 0;
}

extern "C" int64_t tsrl_gail_disc_step_workspace_bytes(int64_t m_pi, int64_t m_exp, int64_t D,
                                                       int64_t A) {
    if (m_pi < 1 || m_exp < 1 || !dims_ok(D, A)) return 0;
    return carve(nullptr, m_pi, m_exp, D + A).bytes;
}

extern "C" int tsrl_gail_disc_step(const tsrl_gail_rows* pi, int64_t m_pi,
                                   const tsrl_gail_rows* expert, int64_t m_exp, int64_t D,
                                   int64_t A, const tsrl_gail_net* net, float* grad, float* out3,
                                   void* ws, int64_t ws_bytes, void* stream) {
    const char* what = "tsrl_gail_disc_step";
    TSRL_CHECK_ARG(m_pi >= 1 && m_exp >= 1 && m_pi < ((int64_t)1 << 31) &&
                   m_exp < ((int64_t)1 << 31),
                   "%s: need 1 <= m_pi, m_exp < 2^31 (got %lld, %lld)", what, (long long)m_pi,
                   (long long)m_exp);
    if (int rc = check_dims(what, D, A, net)) return rc;
    if (int rc = check_rows(what, "policy", pi, D, A)) return rc;
    if (int rc = check_rows(what, "expert", expert, D, A)) return rc;
    TSRL_CHECK_ARG(grad && out3, "%s: null output", what);
    const int64_t need = tsrl_gail_disc_step_workspace_bytes(m_pi, m_exp, D, A);
    TSRL_CHECK_ARG(ws && aligned16(ws) && ws_bytes >= need,
                   "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", what,
                   (long long)need, (long long)ws_bytes);
    const Ws w = carve(ws, m_pi, m_exp, D + A);
    const int grid = step_grid(m_pi, m_exp);
    const int64_t P = n_params_of(D + A);
    hipLaunchKernelGGL(gail_step_kernel, dim3(grid), dim3(TPB), 0, as_stream(stream),
                       rows_of(pi, D), rows_of(expert, D), m_pi, m_exp, (int)D, (int)A,
                       net_of(net), w.part, w.sums, w.dz1);
    TSRL_LAUNCH_CHECK("tsrl_gail_disc_step");
    hipLaunchKernelGGL(gail_fold_kernel, dim3((unsigned)((P + TPB - 1) / TPB)), dim3(TPB), 0,
                       as_stream(stream), w.part, w.sums, grid, P, (double)m_pi, (double)m_exp,
                       grad, out3);
    TSRL_LAUNCH_CHECK("tsrl_gail_disc_step (fold)");
    return 0;
}
