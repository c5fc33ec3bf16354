// The critic ensemble of REDQPolicy (utils/net.py: Critic(Net(concat=True, linear_layer=
// EnsembleLinear), linear_layer=EnsembleLinear)), forward only: per member e and row r
//   q[e, r] = w3[e]^T relu(W2[e]^T relu(W1[e]^T [obs[r] | act[r]] + b1[e]) + b2[e]) + b3[e]
// in one launch.  EnsembleLinear's parameters are read where they lie: weight [E, in, out], bias
// [E, 1, out].  [in, out] is the MFMA B operand's own layout (K runs down a weight column), so
// there is no transposed image and no copy.  obs and act are two arrays with pitches of their
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

template <int H>
__global__ __launch_bounds__(TPB, 1) void ens_fwd_kernel(
    const float* __restrict__ obs, int64_t ldo, const float* __restrict__ act, int64_t lda,
    int64_t b, int D, int A, int E, Net net, const int32_t* __restrict__ members,
    float* __restrict__ q) {
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
    auto put = [&](float* S, const f32x16* acc, const float* bias) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int ft = 32 * (NT * w + j) + c;
            const float bv = bias[ft];
#pragma unroll
            for (int r = 0; r < 16; ++r) S[(rho(r) + 4 * h) * AS + ft] = fmaxf(acc[j][r] + bv, 0.f);
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
        put(H1, acc, b1);
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
        put(H2, acc, b2);
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

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int tsrl_ens_critic_fwd(const float* obs, int64_t ldo, const float* act, int64_t lda,
                                   int64_t b, int64_t D, int64_t A, int64_t H, int64_t E,
                                   const tsrl_ens_net* net, const int32_t* members,
                                   const int32_t* members_host, int64_t S, float* q,
                                   void* stream) {
    const char* what = "tsrl_ens_critic_fwd";
    if (!(H == 128 || H == 256) || D < 1 || A < 0 || D + A > TSRL_ENS_MAX_IN || E < 1 ||
        E > TSRL_ENS_MAX_MEMBERS || b < 1 || b >= ((int64_t)1 << 31)) {
        set_error("%s: takes H in {128, 256}, D + A <= %d, E <= %d and 1 <= b < 2^31 (got H %lld, "
                  "D %lld, A %lld, E %lld, b %lld)", what, TSRL_ENS_MAX_IN, TSRL_ENS_MAX_MEMBERS,
                  (long long)H, (long long)D, (long long)A, (long long)E, (long long)b);
        return TSRL_ERR_ENS_SHAPE;
    }
    TSRL_CHECK_ARG(net && net->w1 && net->b1 && net->w2 && net->b2 && net->w3 && net->b3,
                   "%s: null weight pointer", what);
    TSRL_CHECK_ARG(obs && (act || A == 0) && q, "%s: null pointer", what);
    TSRL_CHECK_ARG(ldo >= D && (A == 0 || lda >= A),
                   "%s: row pitches (%lld, %lld floats) are shorter than the rows (%lld, %lld)",
                   what, (long long)ldo, (long long)lda, (long long)D, (long long)A);
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
    const int64_t tiles = (b + TR - 1) / TR, per = n_cus() / n > 0 ? n_cus() / n : 1;
    const dim3 grid((unsigned)(tiles < per ? tiles : per), (unsigned)n);
    const Net nn{net->w1, net->b1, net->w2, net->b2, net->w3, net->b3};
    auto kern = H == 128 ? ens_fwd_kernel<128> : ens_fwd_kernel<256>;
    hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, as_stream(stream), obs, ldo, act, lda, b, (int)D,
                       (int)A, (int)E, nn, members, q);
    TSRL_LAUNCH_CHECK(what);
    return 0;
}
