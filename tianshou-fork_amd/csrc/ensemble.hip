// The critic ensemble of REDQPolicy (utils/net.py: Critic(Net(concat=True, linear_layer=
// EnsembleLinear), linear_layer=EnsembleLinear)): per member e and row r
//   q[e, r] = w3[e]^T relu(W2[e]^T relu(W1[e]^T [obs[r] | act[r]] + b1[e]) + b2[e]) + b3[e]
// in one launch, and its training pair: the same forward saving h1 / h2, and the backward (the
// section "the backward" below).  EnsembleLinear's parameters are read where they lie: weight
// [E, in, out], bias [E, 1, out].  [in, out] is the MFMA B operand's own layout (K runs down a
// weight column), so there is no transposed image and no copy.  obs and act are two arrays with pitches of their
// own; the layer-1 K loop crosses from one into the other (as gail.hip's does) and no
// concatenated row is written.  With a list of members only those are computed -- REDQ's target
// reads subset_size (2) of the ensemble_size (10) target critics.
//
// Work split.  A workgroup (4 waves) owns (member blockIdx.y, 32-row tile blockIdx.x) and walks
// further tiles of the same member in grid-stride.  Every product is v_mfma_f32_32x32x2f32 on
// f32 operands: lane (c = l & 31, h = l >> 5) supplies A[i = c][k] and B[k][j = c] for k = kk +
// 2h, kk + 2h + 1; C register r of lane (c, h) is element [rho(r) + 4h][c].  Here A is the
// activation tile (i = row) and B the weight chunk (j = feature), so a lane's 16 accumulators
// are 16 rows of one feature and a layer's [32 rows][H] result is H / 32 tiles, H / 128 per wave.
//
// LDS (144 KB at H = 256, 79 KB at 128; one workgroup per CU): h1 and h2 as [32][H + 2] (stride
// 2 mod 32: the 8-byte A reads along a row are conflict-free), a two-deep ring of [32 K-lines][H]
// weight chunks at line stride H + 16 (two lines are 32 banks apart, so the two K halves of a
// wave read disjoint banks), the X tile staged in [32][32 + 2] chunks beside the ring, and b1 |
// b2 | w3.  W1 (Din x H) and W2 (H x H) are never resident: each streams from L2 through the
// ring, the next chunk held in registers while the current one feeds the MFMAs, one barrier per
// chunk.  The K tail of layer 1 is padded in the loop (lines and columns >= Din are zeros in
// LDS), not in memory.  The H -> 1 head is a dot product of h2 against w3 in LDS: 8 threads per
// row, each a fixed stride-8 run of features, then a 3-step butterfly -- a fixed order, so two
// calls on the same inputs are bitwise equal.  Pad rows of a last tile read row b - 1 and write
// nothing.  No host synchronisation and no host read of device memory: legal inside a captured
// graph.
#include <cmath>

#include "tsrl_common.h"

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR = 32;      // rows of a tile
constexpr int TPB = 256;    // 4 waves
constexpr int NWV = TPB / kWave;
constexpr int KC = 32;      // K lines of a weight chunk, columns of a staged X chunk
constexpr int XS = KC + 2;  // stride of an X chunk [32 rows][32 columns]
constexpr int XQ = TR * KC / TPB;  // X elements a thread stages per chunk

template <int H>
struct Map {
    static_assert(H == 128 || H == 256, "ensemble: widths 128 and 256");
    static constexpr int NT = H / (32 * NWV);  // feature tiles per wave
    static constexpr int NF = H / 32;          // float4s a thread moves per weight chunk
    static constexpr int AS = H + 2;           // stride of an activation [32][H]
    static constexpr int WS = H + 16;          // stride of a chunk line
    static constexpr int RB = KC * WS;         // floats of one ring buffer
    static constexpr int H1 = 0, H2 = H1 + TR * AS, RING = H2 + TR * AS, X = RING + 2 * RB,
                         VEC = X + 2 * TR * XS, END = VEC + 3 * H;
    static_assert(RING % 4 == 0 && WS % 4 == 0 && RB % 4 == 0, "float4 chunk stores");
    static_assert(AS % 2 == 0 && X % 2 == 0 && XS % 2 == 0, "float2 operand reads");
    static_assert(END * 4 <= 163840, "ensemble LDS");
};

__device__ __forceinline__ int rho(int r) { return (r & 3) + 8 * (r >> 2); }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float4 ld4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

struct Net {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
};

// nch chunks through the two-deep ring: load(kc) fetches chunk kc into registers, store(slot)
// writes them to ring slot `slot`, use(slot, kc) runs the MFMAs over the chunk in that slot.
// Enters after a barrier that follows the last read of the ring; leaves after one that follows
// its own last read.
template <class Load, class Store, class Use>
__device__ __forceinline__ void stream(int nch, Load load, Store store, Use use) {
    load(0);
    store(0);
    __syncthreads();
    for (int kc = 0; kc < nch; ++kc) {
        const bool more = kc + 1 < nch;
        if (more) load(kc + 1);
        use(kc & 1, kc);
        if (more) store((kc + 1) & 1);
        __syncthreads();
    }
}

// SAVE: the training forward.  The same body (q is bitwise the plain forward's) also writes the
// post-ReLU h1 and h2 of every real row to hs1 / hs2 [E, b, H]; members is null.
template <int H, bool SAVE>
__global__ __launch_bounds__(TPB, 1) void ens_fwd_kernel(
    const float* __restrict__ obs, int64_t ldo, const float* __restrict__ act, int64_t lda,
    int64_t b, int D, int A, int E, Net net, const int32_t* __restrict__ members,
    float* __restrict__ q, float* __restrict__ hs1, float* __restrict__ hs2) {
    using L = Map<H>;
    constexpr int NT = L::NT, NF = L::NF, AS = L::AS, WS = L::WS;
    __shared__ __attribute__((aligned(16))) float sm[L::END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    float *H1 = sm + L::H1, *H2 = sm + L::H2, *RING = sm + L::RING, *X = sm + L::X;
    float* vec = sm + L::VEC;
    const float *b1 = vec, *b2 = vec + H, *w3 = vec + 2 * H;
    const int s = blockIdx.y;
    const int e = members ? members[s] : s;
    float* __restrict__ qs = q + (int64_t)s * b;
    if (e < 0 || e >= E) {  // the host wrapper has validated the list: nothing is read, q is NaN
        for (int64_t r = (int64_t)blockIdx.x * TPB + t; r < b; r += (int64_t)gridDim.x * TPB)
            qs[r] = NAN;
        return;
    }
    const int Din = D + A;
    const float* __restrict__ W1 = net.w1 + (int64_t)e * Din * H;
    const float* __restrict__ W2 = net.w2 + (int64_t)e * H * H;
    const bool v1 = aligned16(net.w1), v2 = aligned16(net.w2);  // H % 4 == 0: every line as the base
    const float b3 = net.b3[e];
    for (int i = t; i < H; i += TPB) {
        vec[i] = net.b1[(int64_t)e * H + i];
        vec[H + i] = net.b2[(int64_t)e * H + i];
        vec[2 * H + i] = net.w3[(int64_t)e * H + i];
    }
    const int64_t tiles = (b + TR - 1) / TR;
    const int nch1 = (Din + KC - 1) / KC;

    float4 pf[NF];  // the next weight chunk: element q is line (t + 256 q) / (H / 4)
    float px[XQ];   // the next X chunk: element q is row (t + 256 q) / 32, column (t + 256 q) % 32
    auto store_w = [&](int slot) {
        float* buf = RING + slot * L::RB;
#pragma unroll
        for (int qd = 0; qd < NF; ++qd) {
            const int i = t + TPB * qd;
            *reinterpret_cast<float4*>(&buf[(i / (H / 4)) * WS + 4 * (i % (H / 4))]) = pf[qd];
        }
    };
    // acc[j] += A[32 rows][KC] (row-major at `a`, stride as) x chunk[KC][features of tile j]
    auto gemm = [&](f32x16* acc, const float* a, int as, const float* buf) {
#pragma unroll 2
        for (int kk = 0; kk < KC; kk += 4) {
            const float2 av = *reinterpret_cast<const float2*>(a + c * as + kk + 2 * h);
            const float* bl = buf + (kk + 2 * h) * WS + 32 * NT * w + c;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                acc[j] = mfma(av.x, bl[32 * j], acc[j]);
                acc[j] = mfma(av.y, bl[WS + 32 * j], acc[j]);
            }
        }
    };
    // C tiles (rows rho(r) + 4h, feature 32 (NT w + j) + c) -> S[row][feature] = relu(. + bias)
    // (SAVE: and -> G[e][row0 + row][feature] for the rows below b)
    auto put = [&](float* S, const f32x16* acc, const float* bias, float* G, int64_t row0) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int ft = 32 * (NT * w + j) + c;
            const float bv = bias[ft];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rho(r) + 4 * h;
                const float v = fmaxf(acc[j][r] + bv, 0.f);
                S[row * AS + ft] = v;
                if (SAVE && row0 + row < b) G[((int64_t)e * b + row0 + row) * H + ft] = v;
            }
        }
    };

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        __syncthreads();  // the previous tile's head has read h2; vec is written
        // 1. h1 = relu([obs | act] W1 + b1): one K loop over both arrays, the tail zero-padded
        f32x16 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        stream(nch1,
            [&](int kc) {
#pragma unroll
                for (int qd = 0; qd < NF; ++qd) {
                    const int i = t + TPB * qd, k = kc * KC + i / (H / 4);
                    pf[qd] = k < Din ? ld4(W1 + (int64_t)k * H + 4 * (i % (H / 4)), v1)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int qd = 0; qd < XQ; ++qd) {
                    const int i = t + TPB * qd, k = kc * KC + (i & 31);
                    int64_t r = row0 + (i >> 5);
                    r = r < b ? r : b - 1;
                    px[qd] = k < D ? obs[r * ldo + k] : k < Din ? act[r * lda + (k - D)] : 0.f;
                }
            },
            [&](int slot) {
                store_w(slot);
                float* xb = X + slot * TR * XS;
#pragma unroll
                for (int qd = 0; qd < XQ; ++qd) {
                    const int i = t + TPB * qd;
                    xb[(i >> 5) * XS + (i & 31)] = px[qd];
                }
            },
            [&](int slot, int) { gemm(acc, X + slot * TR * XS, XS, RING + slot * L::RB); });
        put(H1, acc, b1, hs1, row0);
        // 2. h2 = relu(h1 W2 + b2) (h1 is complete after the stream's first barrier)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        stream(H / KC,
            [&](int kc) {
#pragma unroll
                for (int qd = 0; qd < NF; ++qd) {
                    const int i = t + TPB * qd;
                    pf[qd] = ld4(W2 + (int64_t)(kc * KC + i / (H / 4)) * H + 4 * (i % (H / 4)), v2);
                }
            },
            store_w,
            [&](int slot, int kc) { gemm(acc, H1 + kc * KC, AS, RING + slot * L::RB); });
        put(H2, acc, b2, hs2, row0);
        __syncthreads();
        // 3. q = h2 w3 + b3: 8 threads per row
        {
            const int row = t >> 3, sub = t & 7;
            float sum = 0.f;
#pragma unroll 8
            for (int f = sub; f < H; f += 8) sum = fmaf(H2[row * AS + f], w3[f], sum);
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) sum += __shfl_xor(sum, m, kWave);
            if (sub == 0 && row0 + row < b) qs[row0 + row] = sum + b3;
        }
    }
}

// ---- the backward: tsrl_ens_critic_bwd ---------------------------------------------------------
// Workspace (floats, n = E b H): h1 | h2 (the saving forward's) | dz1 | dz2, each [E, b, H], then
// the per-member action-gradient partials [E, b, A].
//
// Chain phase (ens_chain_kernel, one workgroup per (member, 32-row tile), grid-stride tiles):
//   dz2 = (dq w3^T) o (h2 > 0) on the vector units, dz1 = (dz2 W2^T) o (h1 > 0) and, when asked
//   for, da_e = dz1 W1[e, D:D+A, :]^T on the MFMAs.  These are the transposed uses of [in, out]: K
//   runs along a weight line, so the B operand of lane (c, h) is an 8-byte read along line c.  A
//   chunk is therefore 32 COLUMNS of every line, staged as [H lines][32 + 2]: the line stride is 2
//   mod 32 (the activations' conflict-free pattern), a line's 32 columns are one 128-byte segment
//   of memory, and all H output lines are resident, so wave w owns the output tiles of the
//   forward (NT w ..) and no K split or LDS fold exists.  The ring is two-deep, the next chunk in
//   registers, one barrier per chunk (stream()).  Pad rows of a last tile have dz2 = 0, hence
//   exact zeros everywhere, and write nothing.
// Weight-gradient phase (ens_wgrad_kernel, grid (32-line block of the input | head job, member)):
//   dW[k][n] = sum_r in[r][k] dz[r][n] over all rows in 32-row chunks; A[i = input column][k =
//   row] is the staged input chunk read down its columns, B[k = row][j = n] the dz chunk in the
//   forward's ring layout.  Layer 1's input is the [obs | act] crossing.  The first block of a
//   layer sums its staged dz chunk's columns into db; the head job forms dW3 = h2^T dq and db3.
// ens_da_fold_kernel adds the action partials in member order.  Every sum has a fixed order.
struct Grads {
    float *w1, *b1, *w2, *b2, *w3, *b3;
};

constexpr int TS = KC + 2;                         // line stride of a transposed chunk
constexpr int AQ = TSRL_ENS_MAX_ACT_GRAD * 8 / TPB;  // float4s a thread moves per action chunk

template <int H>
struct ChainMap {
    static constexpr int NF = H / 32;  // float4s a thread moves per W2 chunk [H lines][32]
    static constexpr int AS = H + 2;
    static constexpr int RB = H * TS;
    static constexpr int DZ2 = 0, DZ1 = DZ2 + TR * AS, RING = DZ1 + TR * AS, W3 = RING + 2 * RB,
                         END = W3 + H;
    static_assert(AS % 2 == 0 && RING % 2 == 0 && RB % 2 == 0 && TS % 2 == 0, "float2 reads");
    static_assert(TSRL_ENS_MAX_ACT_GRAD <= H && TSRL_ENS_MAX_ACT_GRAD <= 32 * NWV, "action tiles");
    static_assert(END * 4 <= 163840, "ensemble chain LDS");
};

// columns [col0, col0 + 32) of lines [0, nl) of src (lines ld floats apart; further lines are
// zeros) -> pf: element q is line (t + 256 q) / 8, float4 (t + 256 q) % 8
template <int NQ>
__device__ __forceinline__ void load_lines(float4* pf, const float* __restrict__ src, int ld,
                                           bool vec, int nl, int col0, int t) {
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) {
        const int i = t + TPB * qd, line = i >> 3;
        pf[qd] = line < nl ? ld4(src + (int64_t)line * ld + col0 + 4 * (i & 7), vec)
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

template <int NQ>
__device__ __forceinline__ void store_lines(float* buf, const float4* pf, int t) {
#pragma unroll
    for (int qd = 0; qd < NQ; ++qd) {
        const int i = t + TPB * qd;
        float* p = buf + (i >> 3) * TS + 4 * (i & 7);  // 8-byte aligned: TS is even
        *reinterpret_cast<float2*>(p) = make_float2(pf[qd].x, pf[qd].y);
        *reinterpret_cast<float2*>(p + 2) = make_float2(pf[qd].z, pf[qd].w);
    }
}

// acc[j] += A[32 rows][KC] (row-major at `a`, stride as) x chunk^T, B[k][line] = buf[line TS + k],
// for the 32-line tiles tile0 + j
template <int NTL>
__device__ __forceinline__ void gemm_t(f32x16* acc, const float* a, int as, const float* buf,
                                       int tile0, int c, int h) {
#pragma unroll 2
    for (int kk = 0; kk < KC; kk += 4) {
        const float2 av = *reinterpret_cast<const float2*>(a + c * as + kk + 2 * h);
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            const float2 bv = *reinterpret_cast<const float2*>(
                buf + (32 * (tile0 + j) + c) * TS + kk + 2 * h);
            acc[j] = mfma(av.x, bv.x, acc[j]);
            acc[j] = mfma(av.y, bv.y, acc[j]);
        }
    }
}

template <int H>
__global__ __launch_bounds__(TPB, 1) void ens_chain_kernel(
    int64_t b, int D, int A, Net net, const float* __restrict__ dq,
    const float* __restrict__ hs1, const float* __restrict__ hs2, float* __restrict__ dz1,
    float* __restrict__ dz2, float* __restrict__ dap) {
    using L = ChainMap<H>;
    constexpr int NT = H / (32 * NWV), NF = L::NF, AS = L::AS;
    __shared__ __attribute__((aligned(16))) float sm[L::END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    float *DZ2 = sm + L::DZ2, *DZ1 = sm + L::DZ1, *RING = sm + L::RING, *W3 = sm + L::W3;
    const int e = blockIdx.y, Din = D + A;
    const float* __restrict__ W2 = net.w2 + (int64_t)e * H * H;
    const float* __restrict__ W1a = net.w1 + ((int64_t)e * Din + D) * H;  // the action lines
    const bool v1 = aligned16(net.w1), v2 = aligned16(net.w2);
    const int64_t base = (int64_t)e * b;
    for (int i = t; i < H; i += TPB) W3[i] = net.w3[(int64_t)e * H + i];
    const int64_t tiles = (b + TR - 1) / TR;
    const int na = (A + 31) / 32;  // 32-column tiles of the action gradient, one wave each

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TR;
        __syncthreads();  // W3 is written
        // 1. dz2 = (dq w3^T) o (h2 > 0); pad rows are zeros
        for (int i = t; i < TR * H; i += TPB) {
            const int row = i / H, n = i % H;
            const int64_t r = row0 + row;
            float v = 0.f;
            if (r < b) {
                v = hs2[(base + r) * H + n] > 0.f ? dq[base + r] * W3[n] : 0.f;
                dz2[(base + r) * H + n] = v;
            }
            DZ2[row * AS + n] = v;
        }
        // 2. dz1 = (dz2 W2^T) o (h1 > 0) (DZ2 is complete after the stream's first barrier)
        f32x16 acc[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        float4 pf[NF];
        stream(H / KC, [&](int kc) { load_lines<NF>(pf, W2, H, v2, H, kc * KC, t); },
               [&](int slot) { store_lines<NF>(RING + slot * L::RB, pf, t); },
               [&](int slot, int kc) {
                   gemm_t<NT>(acc, DZ2 + kc * KC, AS, RING + slot * L::RB, NT * w, c, h);
               });
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int ft = 32 * (NT * w + j) + c;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rho(r) + 4 * h;
                float v = 0.f;
                if (row0 + row < b) {
                    v = hs1[(base + row0 + row) * H + ft] > 0.f ? acc[j][r] : 0.f;
                    dz1[(base + row0 + row) * H + ft] = v;
                }
                if (dap) DZ1[row * AS + ft] = v;
            }
        }
        if (!dap) continue;
        // 3. da_e = dz1 W1[e, D:D+A, :]^T: the action lines stream as W2's did, wave w < na owns
        // columns [32 w, 32 w + 32) (DZ1 is complete after the stream's first barrier)
        f32x16 aa;
#pragma unroll
        for (int r = 0; r < 16; ++r) aa[r] = 0.f;
        float4 pa[AQ];
        stream(H / KC, [&](int kc) { load_lines<AQ>(pa, W1a, H, v1, A, kc * KC, t); },
               [&](int slot) { store_lines<AQ>(RING + slot * L::RB, pa, t); },
               [&](int slot, int kc) {
                   if (w < na) gemm_t<1>(&aa, DZ1 + kc * KC, AS, RING + slot * L::RB, w, c, h);
               });
        if (w < na && 32 * w + c < A) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t rr = row0 + rho(r) + 4 * h;
                if (rr < b) dap[(base + rr) * A + 32 * w + c] = aa[r];
            }
        }
    }
}

template <int H>
struct GradMap {
    static constexpr int NF = H / 32, WS = H + 16, RB = KC * WS;
    static constexpr int RING = 0, X = RING + 2 * RB, END = X + 2 * TR * XS;
    static_assert(WS % 4 == 0 && RB % 4 == 0 && END >= TPB, "float4 chunk stores, the head's fold");
};

template <int H>
__global__ __launch_bounds__(TPB, 1) void ens_wgrad_kernel(
    const float* __restrict__ obs, int64_t ldo, const float* __restrict__ act, int64_t lda,
    int64_t b, int D, int A, const float* __restrict__ dq, const float* __restrict__ hs1,
    const float* __restrict__ hs2, const float* __restrict__ dz1, const float* __restrict__ dz2,
    Grads g) {
    using L = GradMap<H>;
    constexpr int NT = H / (32 * NWV), NF = L::NF, WS = L::WS;
    __shared__ __attribute__((aligned(16))) float sm[L::END];
    const int t = threadIdx.x;
    const int w = t >> 6, l = t & 63, h = l >> 5, c = l & 31;
    const int e = blockIdx.y, Din = D + A, n1 = (Din + KC - 1) / KC, n2 = H / KC;
    const int job = blockIdx.x;
    const int64_t base = (int64_t)e * b;
    if (job == n1 + n2) {  // the head: dW3 = h2^T dq and db3 = sum_r dq, rows in order
        const float* __restrict__ gq = dq + base;
        if (t < H) {
            const float* __restrict__ col = hs2 + base * H + t;
            float s = 0.f;
#pragma unroll 8
            for (int64_t r = 0; r < b; ++r) s = fmaf(col[r * H], gq[r], s);
            g.w3[(int64_t)e * H + t] = s;
        }
        // db3 is one number per member: summed in f64 (a butterfly per wave, the four waves in
        // order): its error does not grow with b as an f32 sum's does
        double s = 0.0;
        for (int64_t r = t; r < b; r += TPB) s += (double)gq[r];
        s = wave_sum(s);
        double* part = reinterpret_cast<double*>(sm);
        if (l == 0) part[w] = s;
        __syncthreads();
        if (t == 0) g.b3[e] = (float)(((part[0] + part[1]) + part[2]) + part[3]);
        return;
    }
    const bool first = job < n1;
    const int k0 = (first ? job : job - n1) * KC, nin = first ? Din : H;
    const float* __restrict__ dz = (first ? dz1 : dz2) + base * H;
    const float* __restrict__ hin = hs1 + base * H;  // layer 2's input
    float* __restrict__ dW = first ? g.w1 + (int64_t)e * Din * H : g.w2 + (int64_t)e * H * H;
    const bool vz = aligned16(dz), bias = k0 == 0 && t < H;
    float *RING = sm + L::RING, *X = sm + L::X;

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    float dbs = 0.f;
    float4 pf[NF];  // the next dz chunk: element q is row (t + 256 q) / (H / 4)
    float px[XQ];   // the next input chunk: element q is row (t + 256 q) / 32, column (t + 256 q) % 32
    stream((int)((b + TR - 1) / TR),
        [&](int kc) {
#pragma unroll
            for (int qd = 0; qd < NF; ++qd) {
                const int i = t + TPB * qd;
                const int64_t r = (int64_t)kc * TR + i / (H / 4);
                pf[qd] = r < b ? ld4(dz + r * H + 4 * (i % (H / 4)), vz)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int qd = 0; qd < XQ; ++qd) {
                const int i = t + TPB * qd, k = k0 + (i & 31);
                const int64_t r = (int64_t)kc * TR + (i >> 5);
                float v = 0.f;
                if (r < b && k < nin)
                    v = !first ? hin[r * H + k] : k < D ? obs[r * ldo + k] : act[r * lda + (k - D)];
                px[qd] = v;
            }
        },
        [&](int slot) {
            float* buf = RING + slot * L::RB;
#pragma unroll
            for (int qd = 0; qd < NF; ++qd) {
                const int i = t + TPB * qd;
                *reinterpret_cast<float4*>(&buf[(i / (H / 4)) * WS + 4 * (i % (H / 4))]) = pf[qd];
            }
            float* xb = X + slot * TR * XS;
#pragma unroll
            for (int qd = 0; qd < XQ; ++qd) {
                const int i = t + TPB * qd;
                xb[(i >> 5) * XS + (i & 31)] = px[qd];
            }
        },
        [&](int slot, int) {
            const float* buf = RING + slot * L::RB;
            const float* xb = X + slot * TR * XS;
#pragma unroll 2
            for (int rr = 0; rr < TR; rr += 4) {
                const float a0 = xb[(rr + 2 * h) * XS + c], a1 = xb[(rr + 2 * h + 1) * XS + c];
                const float* bl = buf + (rr + 2 * h) * WS + 32 * NT * w + c;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    acc[j] = mfma(a0, bl[32 * j], acc[j]);
                    acc[j] = mfma(a1, bl[WS + 32 * j], acc[j]);
                }
            }
            if (bias)  // db: the chunk's column t, rows in order (pad rows are zeros)
                for (int r = 0; r < TR; ++r) dbs += buf[r * WS + t];
        });
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int ft = 32 * (NT * w + j) + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + rho(r) + 4 * h;
            if (k < nin) dW[(int64_t)k * H + ft] = acc[j][r];
        }
    }
    if (bias) (first ? g.b1 : g.b2)[(int64_t)e * H + t] = dbs;
}

__global__ void ens_da_fold_kernel(const float* __restrict__ dap, int64_t b, int A, int E,
                                   float* __restrict__ da, int64_t ldda) {
    const int64_t n = b * A;
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        float s = dap[i];
        for (int e = 1; e < E; ++e) s += dap[e * n + i];
        da[(i / A) * ldda + i % A] = s;
    }
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;


namespace {

bool ens_shape_ok(const char* what, int64_t b, int64_t D, int64_t A, int64_t H, int64_t E) {
    if ((H == 128 || H == 256) && D >= 1 && A >= 0 && D + A <= TSRL_ENS_MAX_IN && E >= 1 &&
        E <= TSRL_ENS_MAX_MEMBERS && b >= 1 && b < ((int64_t)1 << 31))
        return true;
    set_error("%s: takes H in {128, 256}, D + A <= %d, E <= %d and 1 <= b < 2^31 (got H %lld, "
              "D %lld, A %lld, E %lld, b %lld)", what, TSRL_ENS_MAX_IN, TSRL_ENS_MAX_MEMBERS,
              (long long)H, (long long)D, (long long)A, (long long)E, (long long)b);
    return false;
}

int ens_check_inputs(const char* what, const float* obs, int64_t ldo, const float* act,
                     int64_t lda, int64_t D, int64_t A, const tsrl_ens_net* net) {
    TSRL_CHECK_ARG(net && net->w1 && net->b1 && net->w2 && net->b2 && net->w3 && net->b3,
                   "%s: null weight pointer", what);
    TSRL_CHECK_ARG(obs && (act || A == 0), "%s: null pointer", what);
    TSRL_CHECK_ARG(ldo >= D && (A == 0 || lda >= A),
                   "%s: row pitches (%lld, %lld floats) are shorter than the rows (%lld, %lld)",
                   what, (long long)ldo, (long long)lda, (long long)D, (long long)A);
    return 0;
}

int ens_check_workspace(const char* what, const void* workspace, int64_t bytes, int64_t b,
                        int64_t H, int64_t E, int64_t A) {
    const int64_t need = tsrl_ens_workspace_bytes(b, H, E, A);
    TSRL_CHECK_ARG(workspace && aligned16(workspace) && bytes >= need,
                   "%s: the workspace needs %lld bytes at a 16-byte boundary (got %lld at %p)",
                   what, (long long)need, (long long)bytes, workspace);
    return 0;
}

// the forward over n members (all E, or the S listed ones); hs1 / hs2 non-null: the saving form
int ens_forward(const char* what, const float* obs, int64_t ldo, const float* act, int64_t lda,
                int64_t b, int64_t D, int64_t A, int64_t H, int64_t E, const tsrl_ens_net* net,
                const int32_t* members, int64_t n, float* q, float* hs1, float* hs2,
                void* stream) {
    const int64_t tiles = (b + TR - 1) / TR, per = n_cus() / n > 0 ? n_cus() / n : 1;
    const dim3 grid((unsigned)(tiles < per ? tiles : per), (unsigned)n);
    const Net nn{net->w1, net->b1, net->w2, net->b2, net->w3, net->b3};
    auto kern = hs1 ? (H == 128 ? ens_fwd_kernel<128, true> : ens_fwd_kernel<256, true>)
                    : (H == 128 ? ens_fwd_kernel<128, false> : ens_fwd_kernel<256, false>);
    hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, as_stream(stream), obs, ldo, act, lda, b, (int)D,
                       (int)A, (int)E, nn, members, q, hs1, hs2);
    TSRL_LAUNCH_CHECK(what);
    return 0;
}

}  // namespace

extern "C" int tsrl_ens_critic_fwd(const float* obs, int64_t ldo, const float* act, int64_t lda,
                                   int64_t b, int64_t D, int64_t A, int64_t H, int64_t E,
                                   const tsrl_ens_net* net, const int32_t* members,
                                   const int32_t* members_host, int64_t S, float* q,
                                   void* stream) {
    const char* what = "tsrl_ens_critic_fwd";
    if (!ens_shape_ok(what, b, D, A, H, E)) return TSRL_ERR_ENS_SHAPE;
    if (int rc = ens_check_inputs(what, obs, ldo, act, lda, D, A, net)) return rc;
    TSRL_CHECK_ARG(q, "%s: null pointer", what);
    TSRL_CHECK_ARG(!members == !members_host,
                   "%s: members needs its host copy (and the copy the list)", what);
    int64_t n = E;
    if (members) {
        TSRL_CHECK_ARG(S >= 1 && S <= E, "%s: need 1 <= S <= E (S %lld, E %lld)", what,
                       (long long)S, (long long)E);
        for (int64_t m = 0; m < S; ++m)
            TSRL_CHECK_ARG(members_host[m] >= 0 && members_host[m] < E,
                           "%s: members[%lld] = %d is outside [0, %lld)", what, (long long)m,
                           (int)members_host[m], (long long)E);
        n = S;
    }
    return ens_forward(what, obs, ldo, act, lda, b, D, A, H, E, net, members, n, q, nullptr,
                       nullptr, stream);
}

extern "C" int64_t tsrl_ens_workspace_bytes(int64_t b, int64_t H, int64_t E, int64_t A) {
    if (b < 1 || H < 1 || E < 1 || A < 0) return 0;
    return 4 * (4 * E * b * H + E * b * A);
}

extern "C" int tsrl_ens_critic_fwd_save(const float* obs, int64_t ldo, const float* act,
                                        int64_t lda, int64_t b, int64_t D, int64_t A, int64_t H,
                                        int64_t E, const tsrl_ens_net* net, float* q,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    const char* what = "tsrl_ens_critic_fwd_save";
    if (!ens_shape_ok(what, b, D, A, H, E)) return TSRL_ERR_ENS_SHAPE;
    if (int rc = ens_check_inputs(what, obs, ldo, act, lda, D, A, net)) return rc;
    TSRL_CHECK_ARG(q, "%s: null pointer", what);
    if (int rc = ens_check_workspace(what, workspace, workspace_bytes, b, H, E, A)) return rc;
    float* ws = static_cast<float*>(workspace);
    return ens_forward(what, obs, ldo, act, lda, b, D, A, H, E, net, nullptr, E, q, ws,
                       ws + E * b * H, stream);
}

extern "C" int tsrl_ens_critic_bwd(const float* obs, int64_t ldo, const float* act, int64_t lda,
                                   int64_t b, int64_t D, int64_t A, int64_t H, int64_t E,
                                   const tsrl_ens_net* net, const float* dq,
                                   const tsrl_ens_grads* grads, float* da, int64_t ldda,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    const char* what = "tsrl_ens_critic_bwd";
    if (!ens_shape_ok(what, b, D, A, H, E)) return TSRL_ERR_ENS_SHAPE;
    if (da && (A < 1 || A > TSRL_ENS_MAX_ACT_GRAD)) {
        set_error("%s: the action gradient takes 1 <= A <= %d (got %lld)", what,
                  TSRL_ENS_MAX_ACT_GRAD, (long long)A);
        return TSRL_ERR_ENS_SHAPE;
    }
    if (int rc = ens_check_inputs(what, obs, ldo, act, lda, D, A, net)) return rc;
    TSRL_CHECK_ARG(dq, "%s: null pointer", what);
    TSRL_CHECK_ARG(grads || da, "%s: neither the weight gradients nor da are asked for", what);
    TSRL_CHECK_ARG(!grads || (grads->w1 && grads->b1 && grads->w2 && grads->b2 && grads->w3 &&
                              grads->b3), "%s: null gradient pointer", what);
    TSRL_CHECK_ARG(!da || ldda >= A, "%s: da's row pitch (%lld floats) is shorter than A (%lld)",
                   what, (long long)ldda, (long long)A);
    if (int rc = ens_check_workspace(what, workspace, workspace_bytes, b, H, E, A)) return rc;
    const int64_t n = E * b * H;
    float* ws = static_cast<float*>(workspace);
    float *hs1 = ws, *hs2 = ws + n, *dz1 = ws + 2 * n, *dz2 = ws + 3 * n, *dap = ws + 4 * n;
    const Net nn{net->w1, net->b1, net->w2, net->b2, net->w3, net->b3};
    hipStream_t st = as_stream(stream);
    {
        const int64_t tiles = (b + TR - 1) / TR, per = n_cus() / E > 0 ? n_cus() / E : 1;
        const dim3 grid((unsigned)(tiles < per ? tiles : per), (unsigned)E);
        auto kern = H == 128 ? ens_chain_kernel<128> : ens_chain_kernel<256>;
        hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, st, b, (int)D, (int)A, nn, dq, hs1, hs2, dz1,
                           dz2, da ? dap : nullptr);
        TSRL_LAUNCH_CHECK(what);
    }
    if (grads) {
        const Grads g{grads->w1, grads->b1, grads->w2, grads->b2, grads->w3, grads->b3};
        const dim3 grid((unsigned)((D + A + KC - 1) / KC + H / KC + 1), (unsigned)E);
        auto kern = H == 128 ? ens_wgrad_kernel<128> : ens_wgrad_kernel<256>;
        hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, st, obs, ldo, act, lda, b, (int)D, (int)A, dq,
                           hs1, hs2, dz1, dz2, g);
        TSRL_LAUNCH_CHECK(what);
    }
    if (da) {
        const int64_t blocks = (b * A + TPB - 1) / TPB;
        hipLaunchKernelGGL(ens_da_fold_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)),
                           dim3(TPB), 0, st, dap, b, (int)A, (int)E, da, ldda);
        TSRL_LAUNCH_CHECK(what);
    }
    return 0;
}
