// The LSTM stack of Recurrent / RecurrentActorProb / RecurrentCritic (utils/net/common.py:288-361,
// continuous.py:238-368): L layers of width H in {64, 128} over x [B, T, Din], of which the nets
// read only the top layer's last step and the final (hidden, cell) [B, L, H].  Gates follow torch's
// order i, f, g, o; the weights are nn.LSTM's own parameters, read where they lie.  Kernels:
//   lstm_fwd_kernel<H, TRAIN>  every time step and every layer of a 32-row tile in one launch.
//   lstm_bwd_seq_kernel<H>     per tile, top layer down and reverse in time: gate gradients,
//                              d h_{t-1} and the gradient of the layer's input.
//   lstm_wgrad_kernel          dW_ih, dW_hh and the bias sums from the gate gradients, one owner
//                              per output element.
//
// Work split.  Rows of the batch are independent, so a workgroup (4 waves) owns 32 rows for the
// whole sequence and nothing is synchronised across the grid.  Every product is
// v_mfma_f32_32x32x2f32 on f32 operands with icm.hip's conventions: lane (c = l & 31, h = l >> 5)
// supplies A[i = c][k] and B[k][j = c] for k = kk + 2h, kk + 2h + 1; C register r of lane (c, h)
// is element [rho(r) + 4h][c].  Forward, the result is [gate row][batch row]: wave w holds hidden
// columns 32 w .. 32 w + 31 of all four gates in four accumulators, so lane (c, h) has i, f, g, o
// of the same sixteen (row c, column) pairs, and the sigmoids, tanh and the cell update happen in
// its registers.  The cell state of every layer stays in registers across t (16 floats per layer);
// only h_t goes back to LDS, as the next step's and the next layer's operand.
//
// Forward per (t, layer): z = [W_ih | W_hh] [in_t | h_{t-1}] is one K loop that crosses from the
// input (x_t, staged with the weights, or the layer below's h_t in LDS) into the layer's own
// h_{t-1} tile.  One layer's [W_ih | W_hh] is 512 KB at H = 128 and cannot stay in the 160 KB of
// LDS, so it streams from L2 through a two-deep ring of [4H lines][16 columns] chunks, the next
// chunk in registers while the current one feeds the MFMAs, one barrier per chunk.  A Din that is
// no multiple of 16 pads the last chunk with zeros in LDS.  LDS at H = 128: h of four layers
// 4 x [32][130], the ring 2 x ([512][18] + x [32][18]), the summed biases: 153 KB.
//
// Workspace of a training forward, floats per (layer, t, row): the four activated gates (4H), the
// cell c_t (H) and h_t (H): 24 H bytes; L T B of them.  The backward recomputes tanh(c_t) only.
// lstm_bwd_seq_kernel overwrites the gates with their gradients dG (same lane, same address) and
// leaves the gradient of a layer's input in that layer's dead c_t slot, where the layer below's
// pass -- the same lane again -- picks it up: no further bytes, and a workspace feeds one backward.
// d h_{t-1} = W_hh^T dz and d in = W_ih^T dz read the weights untransposed in [64 lines][H]
// chunks, K down the gate rows; their results land in the pointwise layout, so d h_{t-1} and d c
// are registers too.  LDS at H = 128: dz [32][514], the ring 2 x [64][130]: 132 KB.
//
// lstm_wgrad_kernel: a workgroup owns 64 gate rows x 64 columns of one layer's [dW_ih | dW_hh]
// (four 32 x 32 tiles) and runs K over the T B rows of dG and of [in_t | h_{t-1}] in order, 32
// rows a step through LDS; column block 0 also sums dG down the rows for both bias gradients.
// No atomics and no partials: two calls on the same inputs are bitwise equal.
//
// expf and tanhf are ROCm's accurate forms (sigmoid = 1 / (1 + expf(-z))).  Pad rows of a last
// tile read row B - 1 and write nothing.
#include "tsrl_common.h"

namespace tsrl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TR = 32;    // batch rows of a tile
constexpr int TPB = 256;  // 4 waves
constexpr int LMAX = 4;
constexpr int KC = 16;    // columns of a forward weight chunk
constexpr int CS = KC + 2;
constexpr int KB = 64;    // lines of a backward weight chunk
constexpr int WT = 64;    // the weight-gradient block is WT x WT
constexpr int WSTR = WT + 1;

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

// four floats at p of which the first `valid` exist (the rest, and all of them for valid <= 0,
// are zeros: the K loop's padding)
__device__ __forceinline__ float4 ldg4(const float* p, int valid, bool vec) {
    if (valid >= 4 && vec) return *reinterpret_cast<const float4*>(p);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid > 0) v.x = p[0];
    if (valid > 1) v.y = p[1];
    if (valid > 2) v.z = p[2];
    if (valid > 3) v.w = p[3];
    return v;
}
__device__ __forceinline__ void put4(float* d, float4 v) {
    *reinterpret_cast<float2*>(d) = make_float2(v.x, v.y);
    *reinterpret_cast<float2*>(d + 2) = make_float2(v.z, v.w);
}
__device__ __forceinline__ float sigm(float z) { return 1.0f / (1.0f + expf(-z)); }

template <class T>
__host__ __device__ __forceinline__ T pick(T const* p, int l) {
    return l == 0 ? p[0] : l == 1 ? p[1] : l == 2 ? p[2] : p[3];
}

// float offsets of the workspace's three arrays, each [L][T][B][.]
struct WsMap {
    int64_t gates, cs, hs, end;
};
__host__ __device__ inline WsMap ws_map(int64_t L, int64_t T, int64_t B, int64_t H) {
    const int64_t n = L * T * B;
    return WsMap{0, n * 4 * H, n * 5 * H, n * 6 * H};
}

struct FwdArgs {
    const float* x;
    int64_t ldb, ldt;
    int B, T, Din, L;
    tsrl_lstm_weights w;
    const float *h0, *c0;
    int64_t s0b, s0l;
    float *hn, *cn;
    int64_t snb, snl;
    float* ws;
};

template <int H>
struct FMap {
    static_assert(H == 64 || H == 128, "lstm: widths 64 and 128");
    static constexpr int NF = H / 32;   // waves with a column tile
    static constexpr int AS = H + 2;    // stride of an h tile [32][H]
    static constexpr int NQ = H / 16;   // float4s of a weight chunk per thread
    static constexpr int WB = 4 * H * CS;      // a ring slot: the weight chunk [4H][16] ...
    static constexpr int SLOT = WB + TR * CS;  // ... and layer 0's x chunk [32][16]
    static constexpr int HS = 0, RING = HS + LMAX * TR * AS, BS = RING + 2 * SLOT,
                         END = BS + LMAX * 4 * H;
    static_assert(RING % 2 == 0 && SLOT % 2 == 0 && WB % 2 == 0, "float2 reads");
    static_assert(END * 4 <= 163840, "lstm forward LDS");
};

template <int H, bool TRAIN>
__global__ __launch_bounds__(TPB, 1) void lstm_fwd_kernel(FwdArgs a) {
    using M = FMap<H>;
    constexpr int NF = M::NF, AS = M::AS, NQ = M::NQ;
    __shared__ __attribute__((aligned(16))) float sm[M::END];
    const int tid = threadIdx.x;
    const int w = tid >> 6, l6 = tid & 63, h = l6 >> 5, c = l6 & 31;
    float *HS = sm + M::HS, *RING = sm + M::RING, *BS = sm + M::BS;
    const int L = a.L, B = a.B, T = a.T;
    const int row0 = blockIdx.x * TR;
    const bool live = row0 + c < B;
    const int64_t rowc = live ? row0 + c : B - 1;
    const bool vx = a.ldb % 4 == 0 && a.ldt % 4 == 0 && aligned16(a.x);
    const WsMap m = ws_map(L, T, B, H);

    float cst[LMAX][16];  // the cell state of (row c, column 32 w + rho(r) + 4 h), per layer
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
        if (l < L) {
            for (int j = tid; j < 4 * H; j += TPB) BS[l * 4 * H + j] = a.w.b_ih[l][j] + a.w.b_hh[l][j];
            for (int i = tid; i < TR * H; i += TPB) {
                const int r = i / H, f = i % H;
                const int64_t rr = row0 + r < B ? row0 + r : B - 1;
                HS[(l * TR + r) * AS + f] = a.h0 ? a.h0[rr * a.s0b + l * a.s0l + f] : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)
            cst[l][r] = (a.c0 && l < L && w < NF)
                ? a.c0[rowc * a.s0b + l * a.s0l + 32 * w + rho(r) + 4 * h] : 0.f;
    }

    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            if (l >= L) continue;
            const int din = l == 0 ? a.Din : H;
            const int nin = (din + KC - 1) / KC, nch = nin + H / KC;
            const float *wih = a.w.w_ih[l], *whh = a.w.w_hh[l];
            const bool vih = din % 4 == 0 && aligned16(wih), vhh = aligned16(whh);
            const float* below = HS + (l > 0 ? l - 1 : 0) * TR * AS;
            float* hl = HS + l * TR * AS;
            const int xr = tid >> 2, xc = 4 * (tid & 3);  // layer 0's x chunk: threads < 128
            const int64_t xrow = row0 + xr < B ? row0 + xr : B - 1;
            float4 pf[NQ + 1];
            // chunk kc < nin: columns 16 kc .. of W_ih (and of x_t); after them W_hh's
            auto load = [&](int kc) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int idx = tid + TPB * q, line = idx >> 2, col = 4 * (idx & 3);
                    if (kc < nin) {
                        const int k0 = kc * KC + col;
                        pf[q] = ldg4(wih + (int64_t)line * din + k0, din - k0, vih);
                    } else {
                        pf[q] = ldg4(whh + (int64_t)line * H + (kc - nin) * KC + col, 4, vhh);
                    }
                }
                if (l == 0 && kc < nin && tid < TR * 4) {
                    const int k0 = kc * KC + xc;
                    pf[NQ] = ldg4(a.x + xrow * a.ldb + (int64_t)t * a.ldt + k0, a.Din - k0, vx);
                }
            };
            auto store = [&](float* slot, int kc) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int idx = tid + TPB * q;
                    put4(slot + (idx >> 2) * CS + 4 * (idx & 3), pf[q]);
                }
                if (l == 0 && kc < nin && tid < TR * 4) put4(slot + M::WB + xr * CS + xc, pf[NQ]);
            };
            f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
            load(0);
            store(RING, 0);
            __syncthreads();
            for (int kc = 0; kc < nch; ++kc) {
                const bool more = kc + 1 < nch;
                if (more) load(kc + 1);
                const float* buf = RING + (kc & 1) * M::SLOT;
                if (w < NF) {
                    const float* bp = kc >= nin ? hl + c * AS + (kc - nin) * KC
                        : l == 0 ? buf + M::WB + c * CS : below + c * AS + kc * KC;
                    const float* ap = buf + (32 * w + c) * CS;
#pragma unroll
                    for (int kk = 0; kk < KC; kk += 4) {
                        const int k = kk + 2 * h;
                        const float2 b = *reinterpret_cast<const float2*>(bp + k);
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const float2 av = *reinterpret_cast<const float2*>(ap + g * H * CS + k);
                            acc[g] = mfma(av.x, b.x, acc[g]);
                            acc[g] = mfma(av.y, b.y, acc[g]);
                        }
                    }
                }
                if (more) store(RING + ((kc + 1) & 1) * M::SLOT, kc + 1);
                __syncthreads();
            }
            // every wave has read h_{t-1}: the gates, the cell and h_t in registers
            if (w < NF) {
                const float* bs = BS + l * 4 * H;
                const int64_t n = ((int64_t)l * T + t) * B + row0 + c;
                float gv[4][16], hv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int f = 32 * w + rho(r) + 4 * h;
                    gv[0][r] = sigm(acc[0][r] + bs[f]);
                    gv[1][r] = sigm(acc[1][r] + bs[H + f]);
                    gv[2][r] = tanhf(acc[2][r] + bs[2 * H + f]);
                    gv[3][r] = sigm(acc[3][r] + bs[3 * H + f]);
                    cst[l][r] = gv[1][r] * cst[l][r] + gv[0][r] * gv[2][r];
                    hv[r] = gv[3][r] * tanhf(cst[l][r]);
                    hl[c * AS + f] = hv[r];
                }
                if (TRAIN && live) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {  // registers 4 q .. 4 q + 3: four adjacent columns
                        const int fo = 32 * w + 8 * q + 4 * h;
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            *reinterpret_cast<float4*>(a.ws + m.gates + n * 4 * H + g * H + fo) =
                                make_float4(gv[g][4 * q], gv[g][4 * q + 1], gv[g][4 * q + 2],
                                            gv[g][4 * q + 3]);
                        *reinterpret_cast<float4*>(a.ws + m.cs + n * H + fo) = make_float4(
                            cst[l][4 * q], cst[l][4 * q + 1], cst[l][4 * q + 2], cst[l][4 * q + 3]);
                        *reinterpret_cast<float4*>(a.ws + m.hs + n * H + fo) =
                            make_float4(hv[4 * q], hv[4 * q + 1], hv[4 * q + 2], hv[4 * q + 3]);
                    }
                }
                if (t == T - 1 && live) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t o = rowc * a.snb + l * a.snl + 32 * w + rho(r) + 4 * h;
                        if (a.hn) a.hn[o] = hv[r];
                        if (a.cn) a.cn[o] = cst[l][r];
                    }
                }
            }
        }
    }
}

struct BwdArgs {
    int B, T, Din, L;
    tsrl_lstm_weights w;
    const float* c0;
    int64_t s0b, s0l;
    const float* dout;
    int64_t ldd;
    float* dx;
    int64_t ldxb, ldxt;
    float* ws;
};

template <int H>
struct BMap {
    static constexpr int NF = H / 32, AS = H + 2, NQ = H / 16;
    static constexpr int DZS = 4 * H + 2;  // stride of dz [32][4H]
    static constexpr int RB = KB * AS;     // a ring buffer: [64 lines][H]
    static constexpr int DZ = 0, RING = DZ + TR * DZS, END = RING + 2 * RB;
    static_assert(KB * H / 4 == NQ * TPB, "a backward chunk is NQ float4s per thread");
    static_assert(END * 4 <= 163840, "lstm backward LDS");
};

// acc[f][row] = sum_j W[j][col0 + f] dz[row][j] over the 4H gate rows j, W's rows `ld` floats
// apart with `ncols` columns (columns past them count as zeros).  Enters after a barrier that
// follows the last read of the ring; leaves after one that follows its own last read.
template <int H>
__device__ __forceinline__ f32x16 wt_dz(const float* W, int ld, int col0, int ncols, bool vec,
                                        const float* DZ, float* RING, int tid) {
    using M = BMap<H>;
    constexpr int NQ = M::NQ, AS = M::AS;
    const int w = tid >> 6, h = (tid & 63) >> 5, c = tid & 31;
    float4 pf[NQ];
    auto load = [&](int kc) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = tid + TPB * q, line = idx / (H / 4), col = col0 + 4 * (idx % (H / 4));
            pf[q] = ldg4(W + (int64_t)(kc * KB + line) * ld + col, ncols - col, vec);
        }
    };
    auto store = [&](float* buf) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int idx = tid + TPB * q;
            put4(buf + (idx / (H / 4)) * AS + 4 * (idx % (H / 4)), pf[q]);
        }
    };
    f32x16 acc = zero16();
    load(0);
    store(RING);
    __syncthreads();
    constexpr int nch = 4 * H / KB;
    for (int kc = 0; kc < nch; ++kc) {
        const bool more = kc + 1 < nch;
        if (more) load(kc + 1);
        const float* buf = RING + (kc & 1) * M::RB;
        if (w < M::NF) {
            const float* ap = buf + 32 * w + c;
            const float* bp = DZ + c * M::DZS + kc * KB;
#pragma unroll 4
            for (int kk = 0; kk < KB; kk += 4) {
                const int k = kk + 2 * h;
                const float2 b = *reinterpret_cast<const float2*>(bp + k);
                acc = mfma(ap[k * AS], b.x, acc);
                acc = mfma(ap[(k + 1) * AS], b.y, acc);
            }
        }
        if (more) store(RING + ((kc + 1) & 1) * M::RB);
        __syncthreads();
    }
    return acc;
}

template <int H>
__global__ __launch_bounds__(TPB, 1) void lstm_bwd_seq_kernel(BwdArgs a) {
    using M = BMap<H>;
    constexpr int NF = M::NF;
    __shared__ __attribute__((aligned(16))) float sm[M::END];
    const int tid = threadIdx.x;
    const int w = tid >> 6, l6 = tid & 63, h = l6 >> 5, c = l6 & 31;
    float *DZ = sm + M::DZ, *RING = sm + M::RING;
    const int L = a.L, B = a.B, T = a.T;
    const int row0 = blockIdx.x * TR;
    const bool live = row0 + c < B;
    const int64_t rowc = live ? row0 + c : B - 1;
    const int64_t TB = (int64_t)T * B;
    const WsMap m = ws_map(L, T, B, H);
    float* ws = a.ws;

    for (int l = L - 1; l >= 0; --l) {
        const float *wih = pick(a.w.w_ih, l), *whh = pick(a.w.w_hh, l);
        float dc[16], dhr[16];  // d c_t and W_hh^T dz_{t+1} of (row c, column 32 w + rho(r) + 4 h)
#pragma unroll
        for (int r = 0; r < 16; ++r) dc[r] = dhr[r] = 0.f;
        for (int t = T - 1; t >= 0; --t) {
            const int64_t n = ((int64_t)l * T + t) * B + rowc;
            __syncthreads();  // the previous step's reads of dz
            if (w < NF) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int fo = 32 * w + 8 * q + 4 * h;
                    float* gp = ws + m.gates + n * 4 * H + fo;
                    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 gi = *reinterpret_cast<const float4*>(gp);
                    const float4 gf = *reinterpret_cast<const float4*>(gp + H);
                    const float4 gg = *reinterpret_cast<const float4*>(gp + 2 * H);
                    const float4 go = *reinterpret_cast<const float4*>(gp + 3 * H);
                    const float4 ct = *reinterpret_cast<const float4*>(ws + m.cs + n * H + fo);
                    const float4 cp = t > 0
                        ? *reinterpret_cast<const float4*>(ws + m.cs + (n - B) * H + fo)
                        : a.c0 ? ldg4(a.c0 + rowc * a.s0b + l * a.s0l + fo, 4, false) : z4;
                    // the layer above left the gradient of its input in its own c_t slot
                    const float4 up = l < L - 1
                        ? *reinterpret_cast<const float4*>(ws + m.cs + (n + TB) * H + fo) : z4;
                    const float4 top = (l == L - 1 && t == T - 1)
                        ? ldg4(a.dout + rowc * a.ldd + fo, 4, false) : z4;
                    const float vi[4] = {gi.x, gi.y, gi.z, gi.w}, vf[4] = {gf.x, gf.y, gf.z, gf.w};
                    const float vg[4] = {gg.x, gg.y, gg.z, gg.w}, vo[4] = {go.x, go.y, go.z, go.w};
                    const float vc[4] = {ct.x, ct.y, ct.z, ct.w}, vp[4] = {cp.x, cp.y, cp.z, cp.w};
                    const float vu[4] = {up.x + top.x, up.y + top.y, up.z + top.z, up.w + top.w};
                    float dz[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * q + j;
                        const float dh = dhr[r] + vu[j], tc = tanhf(vc[j]);
                        const float dct = dc[r] + dh * vo[j] * (1.f - tc * tc);
                        dc[r] = dct * vf[j];
                        dz[0][j] = live ? dct * vg[j] * vi[j] * (1.f - vi[j]) : 0.f;
                        dz[1][j] = live ? dct * vp[j] * vf[j] * (1.f - vf[j]) : 0.f;
                        dz[2][j] = live ? dct * vi[j] * (1.f - vg[j] * vg[j]) : 0.f;
                        dz[3][j] = live ? dh * tc * vo[j] * (1.f - vo[j]) : 0.f;
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 v = make_float4(dz[g][0], dz[g][1], dz[g][2], dz[g][3]);
                        put4(DZ + c * M::DZS + g * H + fo, v);
                        if (live) *reinterpret_cast<float4*>(gp + g * H) = v;
                    }
                }
            }
            __syncthreads();
            if (t > 0) {  // no gradient flows into h0
                const f32x16 acc = wt_dz<H>(whh, H, 0, H, aligned16(whh), DZ, RING, tid);
#pragma unroll
                for (int r = 0; r < 16; ++r) dhr[r] = acc[r];
            }
            if (l > 0) {
                const f32x16 acc = wt_dz<H>(wih, H, 0, H, aligned16(wih), DZ, RING, tid);
                if (w < NF && live) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<float4*>(ws + m.cs + n * H + 32 * w + 8 * q + 4 * h) =
                            make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
                }
            } else if (a.dx) {
                const bool vec = a.Din % 4 == 0 && aligned16(wih);
                for (int p0 = 0; p0 < a.Din; p0 += H) {
                    const f32x16 acc = wt_dz<H>(wih, a.Din, p0, a.Din, vec, DZ, RING, tid);
                    if (w < NF && live) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int f = p0 + 32 * w + rho(r) + 4 * h;
                            if (f < a.Din) a.dx[rowc * a.ldxb + (int64_t)t * a.ldxt + f] = acc[r];
                        }
                    }
                }
            }
        }
    }
}

struct WgArgs {
    const float* x;
    int64_t ldb, ldt;
    int B, T, Din, L, H;
    const float* h0;
    int64_t s0b, s0l;
    tsrl_lstm_grads g;
    const float* ws;
};

__global__ __launch_bounds__(TPB) void lstm_wgrad_kernel(WgArgs a) {
    __shared__ float DG[TR * WSTR], IN[TR * WSTR];
    const int tid = threadIdx.x;
    const int w = tid >> 6, l6 = tid & 63, h = l6 >> 5, c = l6 & 31;
    const int H = a.H, B = a.B, T = a.T;
    const int jbn = 4 * H / WT;
    int blk = blockIdx.x, l = 0, din = a.Din, cbn = (din + H + WT - 1) / WT;
    while (blk >= jbn * cbn) {  // the grid is the layers' blocks in layer order
        blk -= jbn * cbn;
        ++l;
        din = H;
        cbn = (din + H + WT - 1) / WT;
    }
    const int jb = blk / cbn, cb = blk % cbn;
    const int64_t N = (int64_t)T * B;
    const WsMap m = ws_map(a.L, T, B, H);
    const float* dg = a.ws + m.gates + (int64_t)l * N * 4 * H;
    const float* hs = a.ws + m.hs;
    const int wi = w >> 1, wj = w & 1;
    f32x16 acc = zero16();
    float bias = 0.f;
    for (int64_t n0 = 0; n0 < N; n0 += TR) {
#pragma unroll
        for (int q = 0; q < TR * WT / TPB; ++q) {
            const int e = tid + TPB * q, rr = e >> 6, cc = e & 63;
            const int64_t n = n0 + rr;
            float dv = 0.f, iv = 0.f;
            if (n < N) {
                const int64_t t = n / B, b = n % B;
                const int col = cb * WT + cc;
                dv = dg[n * 4 * H + jb * WT + cc];
                if (col < din) {
                    iv = l == 0 ? a.x[b * a.ldb + t * a.ldt + col]
                                : hs[(((int64_t)(l - 1) * T + t) * B + b) * H + col];
                } else if (col - din < H) {
                    const int k = col - din;
                    iv = t > 0 ? hs[(((int64_t)l * T + t - 1) * B + b) * H + k]
                        : a.h0 ? a.h0[b * a.s0b + l * a.s0l + k] : 0.f;
                }
            }
            DG[rr * WSTR + cc] = dv;
            IN[rr * WSTR + cc] = iv;
        }
        __syncthreads();
        if (cb == 0 && tid < WT)
            for (int rr = 0; rr < TR; ++rr) bias += DG[rr * WSTR + tid];
        const float *ap = DG + 32 * wi + c, *bp = IN + 32 * wj + c;
#pragma unroll
        for (int kk = 0; kk < TR; kk += 4) {
            const int k = kk + 2 * h;
            acc = mfma(ap[k * WSTR], bp[k * WSTR], acc);
            acc = mfma(ap[(k + 1) * WSTR], bp[(k + 1) * WSTR], acc);
        }
        __syncthreads();
    }
    float *gih = pick(a.g.w_ih, l), *ghh = pick(a.g.w_hh, l);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = jb * WT + 32 * wi + rho(r) + 4 * h, col = cb * WT + 32 * wj + c;
        if (col < din) gih[(int64_t)j * din + col] = acc[r];
        else if (col - din < H) ghh[(int64_t)j * H + col - din] = acc[r];
    }
    if (cb == 0 && tid < WT) {
        pick(a.g.b_ih, l)[jb * WT + tid] = bias;
        pick(a.g.b_hh, l)[jb * WT + tid] = bias;
    }
}

inline bool shape_ok(int64_t B, int64_t T, int64_t Din, int64_t L, int64_t H) {
    return (H == 64 || H == 128) && L >= 1 && L <= LMAX && T >= 1 && B >= 0 && Din >= 1 &&
        Din <= 512 && B * T < ((int64_t)1 << 31) / LMAX;
}

int check_weights(const char* what, const tsrl_lstm_weights* w, int64_t L) {
    TSRL_CHECK_ARG(w, "%s: null weights", what);
    for (int l = 0; l < L; ++l)
        TSRL_CHECK_ARG(w->w_ih[l] && w->w_hh[l] && w->b_ih[l] && w->b_hh[l],
                       "%s: null weight pointer in layer %d", what, l);
    return 0;
}

}  // namespace
}  // namespace tsrl

using namespace tsrl;

extern "C" int64_t tsrl_lstm_seq_workspace_bytes(int64_t B, int64_t T, int64_t L, int64_t H) {
    if (!shape_ok(B, T, 1, L, H)) return 0;
    return ws_map(L, T, B, H).end * 4;
}

extern "C" int tsrl_lstm_seq_fwd(const float* x, int64_t ldb, int64_t ldt, int64_t B, int64_t T,
                                 int64_t Din, int64_t L, int64_t H, const tsrl_lstm_weights* w,
                                 const float* h0, const float* c0, int64_t s0b, int64_t s0l,
                                 float* hn, float* cn, int64_t snb, int64_t snl, void* ws,
                                 int64_t ws_bytes, void* stream) {
    const char* what = "tsrl_lstm_seq_fwd";
    if (!shape_ok(B, T, Din, L, H)) return TSRL_ERR_LSTM_SHAPE;
    if (B == 0 || (!hn && !cn && !ws)) return 0;
    if (int rc = check_weights(what, w, L)) return rc;
    TSRL_CHECK_ARG(x && (reinterpret_cast<uintptr_t>(x) & 3u) == 0, "%s: x null or misaligned",
                   what);
    TSRL_CHECK_ARG(ldb >= Din && (T == 1 || ldt >= Din),
                   "%s: pitches (%lld, %lld floats) are shorter than the rows (%lld)", what,
                   (long long)ldb, (long long)ldt, (long long)Din);
    TSRL_CHECK_ARG((!h0 && !c0) || (s0b >= H && s0l >= H),
                   "%s: state strides (%lld, %lld) are shorter than H", what, (long long)s0b,
                   (long long)s0l);
    TSRL_CHECK_ARG((!hn && !cn) || (snb >= H && snl >= H),
                   "%s: output strides (%lld, %lld) are shorter than H", what, (long long)snb,
                   (long long)snl);
    if (ws) {
        const int64_t need = tsrl_lstm_seq_workspace_bytes(B, T, L, H);
        TSRL_CHECK_ARG(aligned16(ws) && ws_bytes >= need,
                       "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)",
                       what, (long long)need, (long long)ws_bytes);
    }
    const FwdArgs a{x, ldb, ldt, (int)B, (int)T, (int)Din, (int)L, *w, h0, c0, s0b, s0l,
                    hn, cn, snb, snl, static_cast<float*>(ws)};
    const dim3 grid((unsigned)((B + TR - 1) / TR));
    auto kern = H == 64 ? (ws ? lstm_fwd_kernel<64, true> : lstm_fwd_kernel<64, false>)
                        : (ws ? lstm_fwd_kernel<128, true> : lstm_fwd_kernel<128, false>);
    hipLaunchKernelGGL(kern, grid, dim3(TPB), 0, as_stream(stream), a);
    TSRL_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int tsrl_lstm_seq_bwd(const float* x, int64_t ldb, int64_t ldt, int64_t B, int64_t T,
                                 int64_t Din, int64_t L, int64_t H, const tsrl_lstm_weights* w,
                                 const float* h0, const float* c0, int64_t s0b, int64_t s0l,
                                 const float* d_out, int64_t ldd, const tsrl_lstm_grads* grads,
                                 float* dx, int64_t ldxb, int64_t ldxt, void* ws,
                                 int64_t ws_bytes, void* stream) {
    const char* what = "tsrl_lstm_seq_bwd";
    if (!shape_ok(B, T, Din, L, H)) return TSRL_ERR_LSTM_SHAPE;
    if (B == 0 || !grads) return 0;
    if (int rc = check_weights(what, w, L)) return rc;
    for (int l = 0; l < L; ++l)
        TSRL_CHECK_ARG(grads->w_ih[l] && grads->w_hh[l] && grads->b_ih[l] && grads->b_hh[l],
                       "%s: null gradient pointer in layer %d", what, l);
    TSRL_CHECK_ARG(x && d_out && ldd >= H, "%s: null input or d_out pitch below H", what);
    TSRL_CHECK_ARG(ldb >= Din && (T == 1 || ldt >= Din), "%s: x pitches shorter than the rows",
                   what);
    TSRL_CHECK_ARG((!h0 && !c0) || (s0b >= H && s0l >= H), "%s: state strides shorter than H",
                   what);
    TSRL_CHECK_ARG(!dx || (ldxb >= Din && (T == 1 || ldxt >= Din)),
                   "%s: dx pitches shorter than the rows", what);
    const int64_t need = tsrl_lstm_seq_workspace_bytes(B, T, L, H);
    TSRL_CHECK_ARG(ws && aligned16(ws) && ws_bytes >= need,
                   "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", what,
                   (long long)need, (long long)ws_bytes);
    const BwdArgs a{(int)B, (int)T, (int)Din, (int)L, *w, c0, s0b, s0l, d_out, ldd,
                    dx, ldxb, ldxt, static_cast<float*>(ws)};
    const dim3 grid((unsigned)((B + TR - 1) / TR));
    hipLaunchKernelGGL(H == 64 ? lstm_bwd_seq_kernel<64> : lstm_bwd_seq_kernel<128>, grid,
                       dim3(TPB), 0, as_stream(stream), a);
    TSRL_LAUNCH_CHECK(what);
    const WgArgs g{x, ldb, ldt, (int)B, (int)T, (int)Din, (int)L, (int)H, h0, s0b, s0l, *grads,
                   static_cast<const float*>(ws)};
    const int64_t jbn = 4 * H / WT;
    const int64_t blocks = jbn * ((Din + H + WT - 1) / WT) + (L - 1) * jbn * (2 * H / WT);
    hipLaunchKernelGGL(lstm_wgrad_kernel, dim3((unsigned)blocks), dim3(TPB), 0,
                       as_stream(stream), g);
    TSRL_LAUNCH_CHECK("tsrl_lstm_seq_bwd (weights)");
    return 0;
}
