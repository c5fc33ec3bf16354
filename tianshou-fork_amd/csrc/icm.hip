// The curiosity head of ICMPolicy (tianshou/policy/modelbased/icm.py, utils/net/discrete.py:
// IntrinsicCuriosityModule) over features phi1 = feature_net(obs), phi2 = feature_net(obs_next)
// of width W in {64, 128}:
//   forward model  Linear(W + A, W)-ReLU-Linear(W, W) over phi1 | onehot(act)
//   inverse model  Linear(2 W, W)-ReLU-Linear(W, A)   over phi1 | phi2
// Neither the one-hot nor a concatenated row exists anywhere: the one-hot's share of the first
// layer is the gathered weight column Wf1[:, W + act[r]] added to the accumulators, and the
// inverse model's first layer is one K loop that crosses from the phi1 tile into the phi2 tile
// (as gail.hip crosses from obs into act).  Kernels:
//   icm_kernel<W, false>  forward only: mse[r], act_hat[r, :].
//   icm_kernel<W, true>   one step: forward recomputed, both losses, the backward chain, the
//                         eight parameter gradients, d_phi1 and d_phi2, in one tile visit.
//   icm_fold_kernel       sums the workgroups' partials in workgroup order into the eight
//                         gradient slots and writes (loss, forward, inverse).
//
// Work split.  A tile is 32 rows; a workgroup (4 waves) walks tiles blockIdx.x, + gridDim.x, ...
// Every product is v_mfma_f32_32x32x2f32 on f32 operands with gail.hip's conventions: lane
// (c = l & 31, h = l >> 5) supplies A[i = c][k] and B[k][j = c] for k = kk + 2h, kk + 2h + 1; C
// register r of lane (c, h) is element [rho(r) + 4h][c].  A layer's [W features][32 rows] result
// is W / 32 tiles, one per wave; the 32-wide logits tile is split over K instead (each wave a
// quarter of the hidden units, the four partial tiles summed where the softmax reads them).
//
// LDS (141 KB at W = 128): phi1, phi2, h_f, h_i and e as [32][W] at stride W + 2 (2 mod 32: 8-byte
// row reads and column reads are conflict-free), a two-deep ring of 32 W-float weight chunks, the
// logits partials and g.  The weights (about 260 KB at W = 128) are never resident: each layer
// streams from L2 through the ring, [W lines][32 columns] chunks forward (K runs along a weight
// row) and [32 lines][W columns] chunks backward (K runs down a weight column), the next chunk
// held in registers while the current one feeds the MFMAs, one barrier per chunk.  dz_f overwrites
// h_f after dWf2 has read it and dz_i overwrites h_i after dWi2 has read it; the ReLU masks are
// the signs of the activations being overwritten.  Weight-gradient tiles are 32-row products
// dz^T x read by columns from LDS; dWf1[:, W + a] is the product of dz_f^T with a one-hot tile
// formed in registers from the staged actions.
//
// Gradients leave through one partial per workgroup in the workspace (first tile: store, later
// tiles: the owning thread adds to its own earlier store), folded in workgroup order.  The grid is
// capped at 64 / W x the CU count so that the partials stay below 35 MB.  No atomics: two calls
// on the same inputs are bitwise equal.  Pad rows of a last tile read row M - 1, enter the
// gradients with weight 0, the sums not at all, and write nothing.  A row whose action is outside
// [0, A) gathers column W + 0 and then has its loss terms and gradient seeds set to NaN.
#include "tsrl_common.h"

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR = 32;    // rows of a tile
constexpr int TPB = 256;  // 4 waves
constexpr int NWV = TPB / kWave;
constexpr int KC = 32;    // columns (forward) or lines (backward) of a weight chunk
constexpr int CS = KC + 2;  // stride of a forward chunk [W][32] and of g [32][32]
constexpr int LS = 33;    // stride of a logits partial [32 rows][32 actions] (scalar access)
constexpr int AMAX = 32;

template <int W>
struct Map {
    static_assert(W == 64 || W == 128, "icm: widths 64 and 128");
    static constexpr int NF = W / 32;  // feature tiles; float4s a thread moves per chunk
    static constexpr int AS = W + 2;   // stride of an activation [32][W], of a backward chunk
    static constexpr int RB = W * CS;  // floats of one ring buffer
    static constexpr int PHI1 = 0, PHI2 = PHI1 + TR * AS, HF = PHI2 + TR * AS, HI = HF + TR * AS,
                         E = HI + TR * AS, RING = E + TR * AS, LG = RING + 2 * RB,
                         G = LG + NWV * TR * LS, VEC = G + TR * CS, RS = VEC + 3 * W + AMAX,
                         ACT = RS + 2 * TR, END = ACT + TR;
    static_assert(KC * AS <= RB, "a backward chunk fits a ring buffer");
    static_assert(AS % 2 == 0 && RB % 2 == 0 && RING % 2 == 0 && G % 2 == 0, "float2 reads");
    static_assert(END * 4 <= 163840, "icm LDS");
};

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
struct OneHot {  // [k = row][line = action] of onehot(act), never stored
    const int* act;
    int a;
    __device__ __forceinline__ float2 operator()(int k) const {
        return make_float2(act[k] == a ? 1.f : 0.f, act[k + 1] == a ? 1.f : 0.f);
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

// C tile (features 32 it .., rows c) -> S[c][32 it + rho(r) + 4h] = f(acc, row, feature)
template <class F>
__device__ __forceinline__ void put_tile(float* S, int stride, const f32x16& acc, int it, int c,
                                         int h, F f) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ft = 32 * it + rho(r) + 4 * h;
        S[c * stride + ft] = f(acc[r], c, ft);
    }
}

__device__ __forceinline__ float4 ld4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void put4(float* d, float4 v) {
    *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
}

// parameters() order: forward_model (W1, b1, W2, b2), inverse_model (W1, b1, W2, b2)
struct Net {
    const float *wf1, *bf1, *wf2, *bf2, *wi1, *bi1, *wi2, *bi2;
};
struct Slots {
    float* p[8];
};
struct Offs {  // block b of a partial is floats [o[b], o[b + 1])
    int o[9];
};
__host__ __device__ inline Offs offs_of(int W, int A) {
    Offs f;
    const int n[8] = {W * (W + A), W, W * W, W, W * 2 * W, W, A * W, A};
    f.o[0] = 0;
    for (int b = 0; b < 8; ++b) f.o[b + 1] = f.o[b] + n[b];
    return f;
}

// One chunk of 32 W floats, LINES x COLS, as the thread's NF float4s: element q is line
// (t + 256 q) / (COLS / 4), columns 4 ((t + 256 q) % (COLS / 4)) .. + 3.
template <int W, int COLS, class Src>
__device__ __forceinline__ void chunk_load(float4* pf, int t, Src src) {
#pragma unroll
    for (int q = 0; q < Map<W>::NF; ++q) {
        const int i = t + TPB * q;
        pf[q] = src(i / (COLS / 4), 4 * (i % (COLS / 4)));
    }
}
template <int W, int COLS>
__device__ __forceinline__ void chunk_store(float* buf, const float4* pf, int t) {
#pragma unroll
    for (int q = 0; q < Map<W>::NF; ++q) {
        const int i = t + TPB * q;
        put4(&buf[(i / (COLS / 4)) * (COLS + 2) + 4 * (i % (COLS / 4))], pf[q]);
    }
}

// nch chunks of a weight through the two-deep ring: src(kc, line, col) is four floats of chunk
// kc, use(buf, kc) the MFMAs over the chunk in buf.  Enters after a barrier that follows the last
// read of the ring; leaves after one that follows its own last read.
template <int W, int COLS, class Src, class Use>
__device__ __forceinline__ void stream(float* ring, int nch, int t, Src src, Use use) {
    float4 pf[Map<W>::NF];
    chunk_load<W, COLS>(pf, t, [&](int line, int col) { return src(0, line, col); });
    chunk_store<W, COLS>(ring, pf, t);
    __syncthreads();
    for (int kc = 0; kc < nch; ++kc) {
        const bool more = kc + 1 < nch;
        if (more)
            chunk_load<W, COLS>(pf, t, [&](int line, int col) { return src(kc + 1, line, col); });
        use(ring + (kc & 1) * Map<W>::RB, kc);
        if (more) chunk_store<W, COLS>(ring + ((kc + 1) & 1) * Map<W>::RB, pf, t);
        __syncthreads();
    }
}

template <int W, bool STEP>
__global__ __launch_bounds__(TPB, 1) void icm_kernel(
    const float* __restrict__ phi1, int64_t ld1, const float* __restrict__ phi2, int64_t ld2,
    const int64_t* __restrict__ act, int64_t M, int A, Net net, float* __restrict__ mse_out,
    float* __restrict__ act_hat, float cf, float ci, float* __restrict__ dphi1,
    float* __restrict__ dphi2, float* __restrict__ part, double* __restrict__ sums) {
    using L = Map<W>;
    constexpr int NF = L::NF, AS = L::AS;
    __shared__ __attribute__((aligned(16))) float sm[L::END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    float *PHI1 = sm + L::PHI1, *PHI2 = sm + L::PHI2, *HF = sm + L::HF, *HI = sm + L::HI;
    float *E = sm + L::E, *RING = sm + L::RING, *LG = sm + L::LG, *G = sm + L::G;
    float *vec = sm + L::VEC, *RS = sm + L::RS;
    int* ACT = reinterpret_cast<int*>(sm + L::ACT);
    const float *bf1 = vec, *bf2 = vec + W, *bi1 = vec + 2 * W, *bi2 = vec + 3 * W;
    const int ldf = W + A;  // row pitch of Wf1
    const bool v1 = ld1 % 4 == 0 && aligned16(phi1), v2 = ld2 % 4 == 0 && aligned16(phi2);
    const bool vf1 = ldf % 4 == 0 && aligned16(net.wf1);
    const bool vf2 = aligned16(net.wf2), vi1 = aligned16(net.wi1), vi2 = aligned16(net.wi2);
    const int64_t tiles = (M + TR - 1) / TR;
    const Offs off = offs_of(W, A);
    float* my = STEP ? part + (int64_t)blockIdx.x * off.o[8] : nullptr;

    if (t < W) {
        vec[t] = net.bf1[t];
        vec[W + t] = net.bf2[t];
        vec[2 * W + t] = net.bi1[t];
    }
    if (t < AMAX) vec[3 * W + t] = t < A ? net.bi2[t] : 0.f;
    double s_f = 0.0, s_i = 0.0;  // wave 0, lane = row: the two loss sums

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        const bool first = tile == (int64_t)blockIdx.x;
        // partial element i: stored on the workgroup's first tile, added to afterwards
        auto emit = [&](int i, float v) { my[i] = first ? v : my[i] + v; };
        __syncthreads();  // the previous tile's reads
        // 0. the tile's rows of phi1 and phi2 (pad rows: row M - 1), its actions (-1: invalid)
#pragma unroll
        for (int q = 0; q < NF; ++q) {
            const int i = t + TPB * q, row = i / (W / 4), col = 4 * (i % (W / 4));
            int64_t r = row0 + row;
            r = r < M ? r : M - 1;
            put4(&PHI1[row * AS + col], ld4(phi1 + r * ld1 + col, v1));
            put4(&PHI2[row * AS + col], ld4(phi2 + r * ld2 + col, v2));
        }
        if (t < TR) {
            int64_t r = row0 + t;
            const int64_t a = act[r < M ? r : M - 1];
            ACT[t] = a >= 0 && a < A ? (int)a : -1;
        }
        __syncthreads();
        // 1. z_f^T [f][row] = sum_k Wf1[f][k] phi1[row][k] + Wf1[f][W + a] + bf1[f]
        f32x16 acc = zero16();
        stream<W, KC>(RING, NF, t,
            [&](int kc, int line, int col) {
                return ld4(net.wf1 + (int64_t)line * ldf + kc * KC + col, vf1);
            },
            [&](const float* buf, int kc) {
                if (w < NF) gemm32(acc, KC, h, rowm(buf, CS, 32 * w + c),
                                   rowm(PHI1 + kc * KC, AS, c));
            });
        if (w < NF) {
            const int a = ACT[c] < 0 ? 0 : ACT[c];
            put_tile(HF, AS, acc, w, c, h, [&](float z, int, int f) {
                return fmaxf(z + net.wf1[(int64_t)f * ldf + W + a] + bf1[f], 0.f);
            });
        }
        // 2. z_i^T = Wi1 (phi1 | phi2)^T + bi1: one K loop over both tiles
        acc = zero16();
        stream<W, KC>(RING, 2 * NF, t,
            [&](int kc, int line, int col) {
                return ld4(net.wi1 + (int64_t)line * 2 * W + kc * KC + col, vi1);
            },
            [&](const float* buf, int kc) {
                const float* X = kc < NF ? PHI1 + kc * KC : PHI2 + (kc - NF) * KC;
                if (w < NF) gemm32(acc, KC, h, rowm(buf, CS, 32 * w + c), rowm(X, AS, c));
            });
        if (w < NF)
            put_tile(HI, AS, acc, w, c, h,
                     [&](float z, int, int f) { return fmaxf(z + bi1[f], 0.f); });
        // 3. e = Wf2 h_f + bf2 - phi2 (h_f is complete: every wave has passed step 2's barriers)
        acc = zero16();
        stream<W, KC>(RING, NF, t,
            [&](int kc, int line, int col) {
                return ld4(net.wf2 + (int64_t)line * W + kc * KC + col, vf2);
            },
            [&](const float* buf, int kc) {
                if (w < NF) gemm32(acc, KC, h, rowm(buf, CS, 32 * w + c),
                                   rowm(HF + kc * KC, AS, c));
            });
        if (w < NF)
            put_tile(E, AS, acc, w, c, h, [&](float z, int row, int f) {
                return z + bf2[f] - PHI2[row * AS + f];
            });
        // 4. logits^T [a][row] = Wi2 h_i: Wi2 whole ([32][W], lines >= A zero) into ring buffer 0
        // (it stays there for step 7), K split over the waves
        {
            float4 pf[NF];
            chunk_load<W, W>(pf, t, [&](int line, int col) {
                return line < A ? ld4(net.wi2 + (int64_t)line * W + col, vi2)
                                : make_float4(0.f, 0.f, 0.f, 0.f);
            });
            chunk_store<W, W>(RING, pf, t);
        }
        __syncthreads();
        acc = zero16();
        gemm32(acc, W / NWV, h, rowm(RING + w * (W / NWV), AS, c),
               rowm(HI + w * (W / NWV), AS, c));
#pragma unroll
        for (int r = 0; r < 16; ++r) LG[(w * TR + c) * LS + rho(r) + 4 * h] = acc[r];
        __syncthreads();
        // 5. per row, 8 threads (sub): mse, log-softmax, cross-entropy; e <- cf e, g
        {
            const int row = t >> 3, sub = t & 7, a_row = ACT[row];
            const bool live = row0 + row < M, bad = a_row < 0;
            const float nanv = __builtin_nanf("");
            const float sf = bad ? nanv : live ? cf : 0.f, si = bad ? nanv : live ? ci : 0.f;
            float sq = 0.f;
            for (int f = sub; f < W; f += 8) {
                const float e = E[row * AS + f];
                sq += e * e;
                if (STEP) E[row * AS + f] = sf * e;
            }
            float z[4], zmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // pad logits stay out of the softmax
                const int a = sub + 8 * j;
                z[j] = -INFINITY;
                if (a < A) {
                    z[j] = bi2[a];
                    for (int p = 0; p < NWV; ++p) z[j] += LG[(p * TR + row) * LS + a];
                    if (!STEP && live) act_hat[(row0 + row) * A + a] = z[j];
                }
                zmax = fmaxf(zmax, z[j]);
            }
            float den = 0.f;
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) {
                sq += __shfl_xor(sq, m, kWave);
                zmax = fmaxf(zmax, __shfl_xor(zmax, m, kWave));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) den += expf(z[j] - zmax);  // exp(-inf) = 0
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) den += __shfl_xor(den, m, kWave);
            const float lse = zmax + logf(den);
            if (STEP) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int a = sub + 8 * j;
                    const float p = a < A ? expf(z[j] - zmax) / den : 0.f;
                    G[row * CS + a] = a < A ? si * (p - (a == a_row ? 1.f : 0.f)) : 0.f;
                    if (a == a_row) RS[TR + row] = lse - z[j];
                }
                if (sub == 0) {
                    RS[row] = bad ? nanv : 0.5f * sq;
                    if (bad) RS[TR + row] = nanv;
                }
            } else if (sub == 0 && live) {
                mse_out[row0 + row] = bad ? nanv : 0.5f * sq;
            }
        }
        if (!STEP) continue;
        __syncthreads();
        if (t < TR && row0 + t < M) {
            s_f += (double)RS[t];
            s_i += (double)RS[TR + t];
        }
        // 6. dWi2 = g^T h_i, dWf2 = e^T h_f, db2s; dh_i^T [f][row] = sum_a Wi2[a][f] g[row][a]
        for (int q = w; q < NF; q += NWV) {
            acc = zero16();
            gemm32(acc, TR, h, colm(G, CS, c), colm(HI, AS, 32 * q + c));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = rho(r) + 4 * h;
                if (a < A) emit(off.o[6] + a * W + 32 * q + c, acc[r]);
            }
        }
        for (int q = w; q < NF * NF; q += NWV) {
            const int it = q / NF, jt = q % NF;
            acc = zero16();
            gemm32(acc, TR, h, colm(E, AS, 32 * it + c), colm(HF, AS, 32 * jt + c));
#pragma unroll
            for (int r = 0; r < 16; ++r)
                emit(off.o[2] + (32 * it + rho(r) + 4 * h) * W + 32 * jt + c, acc[r]);
        }
        if (t < W) {
            float s = 0.f;
            for (int r = 0; r < TR; ++r) s += E[r * AS + t];
            emit(off.o[3] + t, s);
        } else if (t - W < A) {  // W + A <= 160 < TPB
            float s = 0.f;
            for (int r = 0; r < TR; ++r) s += G[r * CS + t - W];
            emit(off.o[7] + t - W, s);
        }
        acc = zero16();
        if (w < NF) gemm32(acc, AMAX, h, colm(RING, AS, 32 * w + c), rowm(G, CS, c));
        __syncthreads();  // dWi2 has read h_i, dWf2 h_f, dh_i the ring
        if (w < NF)
            put_tile(HI, AS, acc, w, c, h, [&](float d, int row, int f) {
                return HI[row * AS + f] > 0.f ? d : 0.f;
            });
        // 7. dh_f^T [f][row] = sum_f2 Wf2[f2][f] e[row][f2]; dz_f over h_f
        acc = zero16();
        stream<W, W>(RING, NF, t,
            [&](int kc, int line, int col) {
                return ld4(net.wf2 + (int64_t)(kc * KC + line) * W + col, vf2);
            },
            [&](const float* buf, int kc) {
                if (w < NF) gemm32(acc, KC, h, colm(buf, AS, 32 * w + c),
                                   rowm(E + kc * KC, AS, c));
            });
        if (w < NF)
            put_tile(HF, AS, acc, w, c, h, [&](float d, int row, int f) {
                return HF[row * AS + f] > 0.f ? d : 0.f;
            });
        __syncthreads();
        // 8. dWf1 = dz_f^T (phi1 | onehot), dWi1 = dz_i^T (phi1 | phi2), db1s
        for (int q = w; q < NF * NF; q += NWV) {
            const int it = q / NF, jt = q % NF;
            acc = zero16();
            gemm32(acc, TR, h, colm(HF, AS, 32 * it + c), colm(PHI1, AS, 32 * jt + c));
#pragma unroll
            for (int r = 0; r < 16; ++r)
                emit(off.o[0] + (32 * it + rho(r) + 4 * h) * ldf + 32 * jt + c, acc[r]);
        }
        for (int q = (w + 2) % NWV; q < NF; q += NWV) {  // the waves the dWi2 tiles left idle
            acc = zero16();
            gemm32(acc, TR, h, colm(HF, AS, 32 * q + c), OneHot{ACT, c});
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (c < A) emit(off.o[0] + (32 * q + rho(r) + 4 * h) * ldf + W + c, acc[r]);
        }
        for (int q = w; q < 2 * NF * NF; q += NWV) {
            const int it = q / (2 * NF), jt = q % (2 * NF);
            const float* X = jt < NF ? PHI1 + 32 * jt : PHI2 + 32 * (jt - NF);
            acc = zero16();
            gemm32(acc, TR, h, colm(HI, AS, 32 * it + c), colm(X, AS, c));
#pragma unroll
            for (int r = 0; r < 16; ++r)
                emit(off.o[4] + (32 * it + rho(r) + 4 * h) * 2 * W + 32 * jt + c, acc[r]);
        }
        if (t < 2 * W) {  // 2 W <= TPB
            const float* D = t < W ? HF + t : HI + t - W;
            float s = 0.f;
            for (int r = 0; r < TR; ++r) s += D[r * AS];
            emit(t < W ? off.o[1] + t : off.o[5] + t - W, s);
        }
        // 9. d_phi1^T [k][row] = sum_f Wf1[f][k] dz_f[row][f] + sum_f Wi1[f][k] dz_i[row][f];
        //    d_phi2^T [k][row] = sum_f Wi1[f][W + k] dz_i[row][f] - cf e[row][k]
        auto write_dphi = [&](float* __restrict__ dst, bool minus_e) {
            if (w >= NF || row0 + c >= M) return;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int k = 32 * w + 8 * g + 4 * h;  // registers 4 g .. 4 g + 3
                float4 v = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2],
                                       acc[4 * g + 3]);
                if (minus_e) {
                    const float* e = E + c * AS + k;
                    v = make_float4(v.x - e[0], v.y - e[1], v.z - e[2], v.w - e[3]);
                }
                *reinterpret_cast<float4*>(dst + (row0 + c) * W + k) = v;
            }
        };
        acc = zero16();
        stream<W, W>(RING, 2 * NF, t,
            [&](int kc, int line, int col) {
                return kc < NF
                    ? ld4(net.wf1 + (int64_t)(kc * KC + line) * ldf + col, vf1)
                    : ld4(net.wi1 + (int64_t)((kc - NF) * KC + line) * 2 * W + col, vi1);
            },
            [&](const float* buf, int kc) {
                const float* D = kc < NF ? HF + kc * KC : HI + (kc - NF) * KC;
                if (w < NF) gemm32(acc, KC, h, colm(buf, AS, 32 * w + c), rowm(D, AS, c));
            });
        write_dphi(dphi1, false);
        acc = zero16();
        stream<W, W>(RING, NF, t,
            [&](int kc, int line, int col) {
                return ld4(net.wi1 + (int64_t)(kc * KC + line) * 2 * W + W + col, vi1);
            },
            [&](const float* buf, int kc) {
                if (w < NF) gemm32(acc, KC, h, colm(buf, AS, 32 * w + c),
                                   rowm(HI + kc * KC, AS, c));
            });
        write_dphi(dphi2, true);
    }
    if (STEP && w == 0) {
        s_f = wave_sum(s_f);
        s_i = wave_sum(s_i);
        if (l == 0) {
            sums[2 * (int64_t)blockIdx.x] = s_f;
            sums[2 * (int64_t)blockIdx.x + 1] = s_i;
        }
    }
}

// slot b [j] = sum of the partials in workgroup order; out3 = loss, forward, inverse
__global__ __launch_bounds__(TPB) void icm_fold_kernel(const float* __restrict__ part,
                                                       const double* __restrict__ sums,
                                                       int nparts, Offs off, Slots grads,
                                                       double m, double lr_scale, double wgt,
                                                       float* __restrict__ out3) {
    const int j = blockIdx.x * TPB + threadIdx.x, P = off.o[8];
    if (j < P) {
        double acc = 0.0;
        for (int g = 0; g < nparts; ++g) acc += (double)part[(int64_t)g * P + j];
        int b = 0;
        while (j >= off.o[b + 1]) ++b;
        grads.p[b][j - off.o[b]] = (float)acc;
    }
    if (j == 0) {
        double sf = 0.0, si = 0.0;
        for (int g = 0; g < nparts; ++g) {
            sf += sums[2 * (int64_t)g];
            si += sums[2 * (int64_t)g + 1];
        }
        sf /= m;
        si /= m;
        out3[0] = (float)(((1.0 - wgt) * si + wgt * sf) * lr_scale);
        out3[1] = (float)sf;
        out3[2] = (float)si;
    }
}

inline int64_t tiles_of(int64_t m) { return (m + TR - 1) / TR; }
inline int step_grid(int64_t m, int64_t W) {
    const int64_t cap = (int64_t)n_cus() * 64 / W, tiles = tiles_of(m);
    return (int)(tiles < cap ? tiles : cap > 0 ? cap : 1);
}
inline bool dims_ok(int64_t W, int64_t A) { return (W == 64 || W == 128) && A >= 1 && A <= AMAX; }

Net net_of(const tsrl_icm_net* s) {
    return Net{s->wf1, s->bf1, s->wf2, s->bf2, s->wi1, s->bi1, s->wi2, s->bi2};
}

int check_common(const char* what, const float* phi1, int64_t ld1, const float* phi2,
                 int64_t ld2, const int64_t* act, int64_t M, int64_t W, int64_t A,
                 const tsrl_icm_net* net) {
    TSRL_CHECK_ARG(M >= 0 && M < ((int64_t)1 << 31), "%s: need 0 <= M < 2^31 (got %lld)", what,
                   (long long)M);
    TSRL_CHECK_ARG(dims_ok(W, A), "%s: need W in {64, 128} and 1 <= A <= 32 (got %lld, %lld)",
                   what, (long long)W, (long long)A);
    TSRL_CHECK_ARG(net && net->wf1 && net->bf1 && net->wf2 && net->bf2 && net->wi1 && net->bi1 &&
                   net->wi2 && net->bi2, "%s: null weight pointer", what);
    if (M == 0) return 0;
    TSRL_CHECK_ARG(phi1 && phi2 && act, "%s: null input", what);
    TSRL_CHECK_ARG(ld1 >= W && ld2 >= W,
                   "%s: row pitches (%lld, %lld floats) are shorter than the rows (%lld)", what,
                   (long long)ld1, (long long)ld2, (long long)W);
    TSRL_CHECK_ARG(((reinterpret_cast<uintptr_t>(phi1) | reinterpret_cast<uintptr_t>(phi2)) &
                    3u) == 0, "%s: phi1 and phi2 must be 4-byte aligned", what);
    return 0;
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_icm_head_fwd(const float* phi1, int64_t ld1, const float* phi2, int64_t ld2,
                                 const int64_t* act, int64_t M, int64_t W, int64_t A,
                                 const tsrl_icm_net* net, float* mse, float* act_hat,
                                 void* stream) {
    const char* what = "tsrl_icm_head_fwd";
    if (int rc = check_common(what, phi1, ld1, phi2, ld2, act, M, W, A, net)) return rc;
    if (M == 0) return 0;
    TSRL_CHECK_ARG(mse && act_hat, "%s: null output", what);
    const int64_t tiles = tiles_of(M), cap = n_cus();
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
    auto kern = W == 64 ? icm_kernel<64, false> : icm_kernel<128, false>;
    hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, as_stream(stream), phi1, ld1, phi2, ld2, act, M,
                       (int)A, net_of(net), mse, act_hat, 0.f, 0.f, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, (double*)nullptr);
    TSRL_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int64_t tsrl_icm_head_step_workspace_bytes(int64_t M, int64_t W, int64_t A) {
    if (M < 1 || M >= ((int64_t)1 << 31) || !dims_ok(W, A)) return 0;
    const int64_t grid = step_grid(M, W);
    return grid * 16 + grid * (int64_t)offs_of((int)W, (int)A).o[8] * 4;
}

extern "C" int tsrl_icm_head_step(const float* phi1, int64_t ld1, const float* phi2, int64_t ld2,
                                  const int64_t* act, int64_t M, int64_t W, int64_t A,
                                  const tsrl_icm_net* net, const tsrl_icm_grads* grads,
                                  float* d_phi1, float* d_phi2, double lr_scale,
                                  double forward_loss_weight, float* out3, void* ws,
                                  int64_t ws_bytes, void* stream) {
    const char* what = "tsrl_icm_head_step";
    if (int rc = check_common(what, phi1, ld1, phi2, ld2, act, M, W, A, net)) return rc;
    if (M == 0) return 0;
    TSRL_CHECK_ARG(grads && grads->wf1 && grads->bf1 && grads->wf2 && grads->bf2 && grads->wi1 &&
                   grads->bi1 && grads->wi2 && grads->bi2 && d_phi1 && d_phi2 && out3,
                   "%s: null output", what);
    TSRL_CHECK_ARG(aligned16(d_phi1) && aligned16(d_phi2),
                   "%s: d_phi1 and d_phi2 must be 16-byte aligned", what);
    const int64_t need = tsrl_icm_head_step_workspace_bytes(M, W, A);
    TSRL_CHECK_ARG(ws && aligned16(ws) && ws_bytes >= need,
                   "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", what,
                   (long long)need, (long long)ws_bytes);
    const int grid = step_grid(M, W);
    const Offs off = offs_of((int)W, (int)A);
    double* sums = static_cast<double*>(ws);
    float* part = reinterpret_cast<float*>(sums + 2 * (int64_t)grid);
    const float cf = (float)(lr_scale * forward_loss_weight / (double)M);
    const float ci = (float)(lr_scale * (1.0 - forward_loss_weight) / (double)M);
    auto kern = W == 64 ? icm_kernel<64, true> : icm_kernel<128, true>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(TPB), 0, as_stream(stream), phi1, ld1, phi2, ld2,
                       act, M, (int)A, net_of(net), (float*)nullptr, (float*)nullptr, cf, ci,
                       d_phi1, d_phi2, part, sums);
    TSRL_LAUNCH_CHECK(what);
    const Slots slots{{grads->wf1, grads->bf1, grads->wf2, grads->bf2, grads->wi1, grads->bi1,
                       grads->wi2, grads->bi2}};
    hipLaunchKernelGGL(icm_fold_kernel, dim3((unsigned)((off.o[8] + TPB - 1) / TPB)), dim3(TPB),
                       0, as_stream(stream), part, sums, grid, off, slots, (double)M, lr_scale,
                       forward_loss_weight, out3);
    TSRL_LAUNCH_CHECK("tsrl_icm_head_step (fold)");
    return 0;
}
