// Forward for training and backward of the encoder, ModelDown.qs_net (the reference's src/torchmodel.py:84-104), at the Dynamic-dSprites
// geometry 1 x 64 x 64, and the gradient of F_down at the latent: with train_dec_head.hip and train_dec.hip the gradient of
// mean(F_down) of train_model_down (torchloss.py:90-98) with respect to every parameter of ModelDown.
//     x0 = o [1][64][64]
//     y1 = relu(Conv2d( 1, 32, k3, s2)(x0))   [32][31][31]
//     y2 = relu(Conv2d(32, 32, k3, s2)(y1))   [32][15][15]
//     y3 = relu(Conv2d(32, 64, k3, s2)(y2))   [64][ 7][ 7]
//     y4 = relu(Conv2d(64, 64, k3, s2)(y3))   [64][ 3][ 3]     flattened in the reference's order c 9 + p
//     h1 = relu(W9 y4 + b) keep0 2,  h2 = relu(W12 h1 + b) keep1 2,  h3 = relu(W15 h2 + b) keep2 2      [256]
//     out = W18 h3 + b = (mean[10], logvar[10])
// qs_net.9.weight is [256][576], the engine's documented correction of the shipped defect.  W [Cout][Cin][3][3] / [out][in] row-major comes
// from the raw device copy of the parameters (flat, parameters() order, EQ_* offsets of kernels.h).  No padding: every extent is odd
// (31, 15, 7, 3; 961, 225, 49, 9 positions), row 63 and column 63 of the image are never read, and every tile is ragged: a padding lane
// feeds exact zeros into both MFMA operands and its address is clamped to element 0 of its own image.
//
// Dropout: the keep mask of head layer li = 0..2 is the forward encoder's (dense_head(enc = true) / k_head), draw for draw: tag TAG_ENC +
// li, block f >> 7, word (f >> 5) & 3, bit f & 31, the call's row / stream / stage.  mean / logvar agree with efe_encoder to rounding.
//
// Kernels (one row group of at most DEC_TAIL_ROWS = 64 rows per launch):
//   k_enc_conv1  : layer 1 (Cin = 1) on the VALU, one thread per output.
//   k_enc_conv<CI, CO, HIN>  : layers 2..4 on v_mfma_f32_16x16x4_f32: one wave = 16 output channels x 16 consecutive output positions
//                  (flattened oy HOUT + ox), K = the input channels, per tap.
//   k_ench_fwd   : the dense head, one workgroup per 16-row tile, activations in LDS (49 920 B) and stored to h1..h3, mean, logvar.
//   k_ench_bwd   : the head backward over one 16-row tile from the upstream pair (g_mean, g_logvar), built of train_mlp.h's passes; ends in
//                  g4 = dL / da4 = (g_0 W9) [y4 > 0].  LDS 56 064 B: G3 | A | U, U = a 256-wide activation, then the 576-wide y4 tile.
//   k_enc_wgrad<CI, CO, HIN> : dW[co][ci][tap] = sum_{m, oy, ox} g[m][co][oy][ox] x[m][ci][2 oy + ky][2 ox + kx], MFMA with K = the
//                  positions; one wave owns a 16 co x 16 ci tile for all nine taps (train_conv.h's wgrad_mfma).
//   k_enc_w1     : the 288 weights of layer 1, one workgroup per (co, slab) (train_conv.h's wgrad_valu).
//   k_conv_bias (train_dec.hip, launch_conv_bias) : db[co] = sum g, per (co, slab).
//   k_enc_dx<CI, CO, HIN>    : dx[ci][iy][ix] = (sum_{co, ky, kx : iy = 2 oy + ky, ix = 2 ox + kx} g[co][oy][ox] W[co][ci][ky][kx]) [x > 0]:
//                  one wave = 16 input channels x 16 positions of ONE input parity class (iy & 1, ix & 1), which fixes the taps that reach
//                  it (4, 2, 2 or 1 of the 9), K = the output channels per tap.  No gradient with respect to the image is formed.
//   k_down_latent: (g_mean, g_logvar) = d mean(F_down) / d (qs1_mean, qs1_logvar), one thread per (row, k).
//   k_slab_sum (train.hip) : gradient = ascending sum of the slabs.
//
// Forward order: conv1 one 9-term fma chain (ky, kx ascending) + bias.  Layers 2..4: per kernel row ky three chains (kx = 0, 1, 2) over the
// input channels ascending, sum = ((sum + c_0) + c_1) + c_2, ky ascending; then + bias.  The head: train_mlp.h's chain with EIGHT
// accumulators (K = 576: 36 chunks; K = 256: 16).  The data gradient: per tap in (ky, kx) ascending order one chain over the output
// channels, sum = sum + tap.  Features 20..31 of the last layer's padded tile feed exact zeros into both operands (never what lies
// behind qs_net.18.weight in the flat copy).
//
// Reduction-order contract of the parameter gradient (a function of M alone, no float atomics; every (element, slab) has ONE owning
// thread; two identical calls give identical bits):
//   rows     : row group g = rows 64 g .. 64 g + 63 (DEC_TAIL_ROWS, so that the composed call interleaves with the decoder's groups),
//              16-row tile t = rows 16 t .. 16 t + 15; rows >= M contribute exact zeros.
//   convs    : GC = min(M, ENC_CONV_SLABS = 32) slabs of ENC_CONV_P = 64 992 floats; row m belongs to slab m mod GC (at most 2 images per
//              slab and group).  Chunk, image, group and slab order: train_conv.h; the last chunk of an image is ragged.
//   head     : GH = min(ceil(M / 16), ENC_HEAD_SLABS = 4) slabs of ENC_HEAD_P = 284 436 floats; tile t adds its 16-term chain (db: the
//              sequential sum of its rows) to slab t mod 4, tiles ascending (train_mlp.h's tile and gate rules).
//   gradient = ((slab_0 + slab_1) + slab_2) + ... ascending (k_slab_sum).
// The per-row outputs (mean, logvar, y1..y4, h1..h3, g_mean, g_logvar) depend on that row and its global row id only.
#include "train_mlp.h"
#include "train_conv.h"

namespace efe {

using namespace mlp;

namespace {

constexpr int HLD = 256 + 4;       // LDS row stride of a 256-wide activation
constexpr int XLD = 576 + 4;       // ... of the y4 tile
constexpr int GLD = 32 + 4;        // ... of the upstream tile (mean | logvar, zero from column 20)

// a [16][256] activation tile of the group into LDS, zero beyond the group's rows; thread = column
__device__ __forceinline__ void load_tile256(float* dst, const float* src, int r0, int rows, int tid) {
#pragma unroll 4
    for (int r = 0; r < TR; ++r) dst[r * HLD + tid] = r0 + r < rows ? src[(size_t)(r0 + r) * 256 + tid] : 0.0f;
}

}  // namespace

// ---- forward -----------------------------------------------------------------------------------------------------------------
// layer 1: o [rows][64][64] -> y1 [rows][32][31][31]; one thread per output
__global__ void __launch_bounds__(256) k_enc_conv1(const float* __restrict__ o, const float* __restrict__ w, float* __restrict__ y1, int rows) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 32 * 961) return;
    const int r = i / (32 * 961), t = i - r * (32 * 961), co = t / 961, pos = t - co * 961, oy = pos / 31, ox = pos - oy * 31;
    const float* x = o + (size_t)r * 4096 + (2 * oy) * 64 + 2 * ox;          // (last pixel read: row 62, column 62)
    const float* wp = w + EQ_W1 + co * 9;
    float c = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) c = fmaf(x[ky * 64 + kx], wp[3 * ky + kx], c);
    y1[i] = relu_nan(c + w[EQ_B1 + co]);
}

// layers 2..4: x [rows][CI][HIN][HIN] -> y = relu(conv + bias) [rows][CO][HOUT][HOUT], HOUT = (HIN - 1) / 2
template <int CI, int CO, int HIN>
__global__ void __launch_bounds__(256) k_enc_conv(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                  float* __restrict__ y, int rows) {
#pragma clang fp contract(off)
    constexpr int HOUT = (HIN - 1) / 2, HW = HOUT * HOUT, PT = (HW + 15) / 16, PER_ROW = (CO / 16) * PT;
    static_assert(CI % 4 == 0 && CO % 16 == 0 && 2 * HOUT + 1 == HIN, "whole channel tiles, odd extent");
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW, t_ = task - r * PER_ROW, pt = t_ % PT, co0 = 16 * (t_ / PT);
    const int pos = 16 * pt + n;
    const bool ok = pos < HW;
    const int pc = ok ? pos : 0, oy = pc / HOUT, ox = pc - oy * HOUT;
    const float* xr = x + (size_t)r * CI * HIN * HIN + (2 * oy) * HIN + 2 * ox;       // B(k = ci, j = position n)
    const float* wr = W + (size_t)(co0 + n) * CI * 9;                                 // A(i = co n, k = ci)
    f32x4 total = (f32x4)(0.f);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        f32x4 c[3] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll 2
        for (int k0 = 0; k0 < CI; k0 += 4) {
            const int k = k0 + q;
            const float* xp = xr + (size_t)k * HIN * HIN + ky * HIN;
            const float* wp = wr + k * 9 + 3 * ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                float bv = xp[kx];
                bv = ok ? bv : 0.0f;
                c[kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[kx], bv, c[kx], 0, 0, 0);
            }
        }
        total = ((total + c[0]) + c[1]) + c[2];
    }
    if (!ok) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int co = co0 + 4 * q + e;                                               // D(i = 4 q + e, j = n)
        y[((size_t)r * CO + co) * HW + pos] = relu_nan(total[e] + bias[co]);
    }
}

// the dense head: grid = ceil(rows / 16)
__global__ void __launch_bounds__(256) k_ench_fwd(const EncTrainArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float H[3 * TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, row = r0 + n;
    const bool rok = row < a.rows;
#pragma unroll 1
    for (int l = 0; l < 4; ++l) {
        const gfloat* W = (const gfloat*)a.w + (l == 0 ? EQ_W9 : l == 1 ? EQ_W12 : l == 2 ? EQ_W15 : EQ_W18);
        const gfloat* B = (const gfloat*)a.w + (l == 0 ? EQ_B9 : l == 1 ? EQ_B12 : l == 2 ? EQ_B15 : EQ_B18);
        const int O = l == 3 ? 20 : 256, NT = l == 3 ? 2 : 16;
        float* hl = l == 0 ? a.h1 : l == 1 ? a.h2 : a.h3;
#pragma unroll 1
        for (int t = w; t < NT; t += 4) {
            const int f0 = 16 * t;
            f32x4 sum;
            if (l == 0) {                     // K = 576: x = y4 from memory, zero beyond the group's rows
                const float* xp = a.y4 + (size_t)(rok ? row : 0) * 576 + 4 * q;                          // B(k, j = row): y4[n][16 c + 4 q + s]
                const float4* Wp = reinterpret_cast<const float4*>((const float*)W + (size_t)(f0 + n) * 576 + 4 * q);
                sum = contract<8, 36>([&](int c) { return Wp[4 * c]; }, [&](int c) {                     // A(i = feature, k): W[f0 + n][16 c + 4 q + s]
                    float4 bv = *reinterpret_cast<const float4*>(xp + 16 * c);
                    if (!rok) bv = make_float4(0.f, 0.f, 0.f, 0.f);
                    return bv;
                });
            } else {                          // K = 256; the last layer's features 20..31 feed zeros, read from row 0
                const float* x = H + (l - 1) * TR * HLD + n * HLD + 4 * q;
                const bool fin = f0 + n < O;
                const float4* Wp = reinterpret_cast<const float4*>((const float*)W + (size_t)(fin ? f0 + n : 0) * 256 + 4 * q);
                sum = contract<8, 16>([&](int c) {
                    float4 av = Wp[4 * c];
                    if (!fin) av = make_float4(0.f, 0.f, 0.f, 0.f);
                    return av;
                }, [&](int c) { return *reinterpret_cast<const float4*>(x + 16 * c); });
            }
            if (l < 3) {
                const uint32_t word = mask_word(mask_block(a.key, TAG_ENC + (uint32_t)l, (uint32_t)(f0 >> 7), (uint32_t)row), f0);
                const float4 out = fwd_epilogue(sum, B, f0, q, 256, true, true, word);                   // D(i = 4 q + e, j = n)
                *reinterpret_cast<float4*>(H + l * TR * HLD + n * HLD + f0 + 4 * q) = out;
                if (rok) *reinterpret_cast<float4*>(hl + (size_t)row * 256 + f0 + 4 * q) = out;
            } else {
                const float4 out = fwd_epilogue(sum, B, f0, q, 20, false, false, 0u);
                const float o4[4] = {out.x, out.y, out.z, out.w};
                if (rok)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int f = f0 + 4 * q + e;
                        if (f < 10) a.mean[(size_t)row * 10 + f] = o4[e];
                        else if (f < 20) a.logvar[(size_t)row * 10 + f - 10] = o4[e];
                    }
            }
        }
        __syncthreads();
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------
// the dense head over one 16-row tile; slab = the tile's index in its row group.  grid = ceil(rows / 16)
// LDS: G3 = g_3 (upstream) | A = x_3 = h3, then g_2 | U = x_2 = h2, then g_1; A = x_1 = h1, then g_0; U = x_0 = y4 [16][576], then g4
__global__ void __launch_bounds__(256) k_ench_bwd(const EncTrainArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float G3[TR * GLD];
    __shared__ __attribute__((aligned(16))) float A[TR * HLD];
    __shared__ __attribute__((aligned(16))) float U[TR * XLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR;
    const bool first = a.first != 0;
    const gfloat* wt = (const gfloat*)a.w;
    gfloat* slab = (gfloat*)a.hslabs + (size_t)blockIdx.x * ENC_HEAD_P;         // element EQ_x of the gradient is slab[EQ_x - EQ_W9]
    {
        const int r = tid >> 4;
        const bool rok = r0 + r < a.rows;
#pragma unroll
        for (int c = tid & 15; c < 32; c += 16) {
            float v = 0.0f;
            if (rok && c < 10) v = a.g_mean[(size_t)(r0 + r) * 10 + c];
            else if (rok && c < 20) v = a.g_logvar[(size_t)(r0 + r) * 10 + c - 10];
            G3[r * GLD + c] = v;
        }
    }
    load_tile256(A, a.h3, r0, a.rows, tid);
    load_tile256(U, a.h2, r0, a.rows, tid);
    __syncthreads();
    // layer 3 (qs_net.18, 20 outputs in a 32-wide tile, no gate on its output)
    dw_pass(G3, GLD, A, HLD, 20, 256, slab + (EQ_W18 - EQ_W9), first, w, n, q);
    db_pass(G3, GLD, 20, slab + (EQ_B18 - EQ_W9), first, tid);
    __syncthreads();                                                            // dW has consumed x: it may now be overwritten
    dprev_pass<8, 2, true>(G3, GLD, A, HLD, wt + EQ_W18, 256, 2.0f, true, w, n, q, 20);
    __syncthreads();
    // layer 2 (qs_net.15)
    dw_pass(A, HLD, U, HLD, 256, 256, slab + (EQ_W15 - EQ_W9), first, w, n, q);
    db_pass(A, HLD, 256, slab + (EQ_B15 - EQ_W9), first, tid);
    __syncthreads();
    dprev_pass<8, 16>(A, HLD, U, HLD, wt + EQ_W15, 256, 2.0f, true, w, n, q);
    __syncthreads();
    load_tile256(A, a.h1, r0, a.rows, tid);
    __syncthreads();
    // layer 1 (qs_net.12)
    dw_pass(U, HLD, A, HLD, 256, 256, slab + (EQ_W12 - EQ_W9), first, w, n, q);
    db_pass(U, HLD, 256, slab + (EQ_B12 - EQ_W9), first, tid);
    __syncthreads();
    dprev_pass<8, 16>(U, HLD, A, HLD, wt + EQ_W12, 256, 2.0f, true, w, n, q);
    __syncthreads();
#pragma unroll 1
    for (int i = tid; i < TR * 576; i += 256) {
        const int r = i / 576, c = i - r * 576;
        U[r * XLD + c] = r0 + r < a.rows ? a.y4[(size_t)(r0 + r) * 576 + c] : 0.0f;
    }
    __syncthreads();
    // layer 0 (qs_net.9): the gate into the conv stack is [y4 > 0], keep = 1
    dw_pass(A, HLD, U, XLD, 256, 576, slab + (EQ_W9 - EQ_W9), first, w, n, q);
    db_pass(A, HLD, 256, slab + (EQ_B9 - EQ_W9), first, tid);
    __syncthreads();
    dprev_pass<8, 16>(A, HLD, U, XLD, wt + EQ_W9, 576, 1.0f, true, w, n, q);
    __syncthreads();
#pragma unroll 1
    for (int i = tid; i < TR * 576; i += 256) {
        const int r = i / 576, c = i - r * 576;
        if (r0 + r < a.rows) a.g4[(size_t)(r0 + r) * 576 + c] = U[r * XLD + c];
    }
}

// x [rows][CI][HIN][HIN], g [rows][CO][HOUT][HOUT] -> slab[(co CI + ci) 9 + tap]; grid ((CO / 16) (CI / 16) / 4, G)
template <int CI, int CO, int HIN>
__global__ void __launch_bounds__(256) k_enc_wgrad(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ slab_w,
                                                   int rows, int first) {
#pragma clang fp contract(off)
    constexpr int HOUT = (HIN - 1) / 2, HW = HOUT * HOUT, XW = HIN * HIN;
    static_assert((CI / 16) * (CO / 16) % 4 == 0 && 2 * HOUT + 1 == HIN, "whole workgroups, odd extent");
    const int n = threadIdx.x & 15;
    const int pair = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int co0 = 16 * (pair / (CI / 16)), ci0 = 16 * (pair % (CI / 16));
    // a position >= HW of the ragged last chunk: zero into both operands, the address clamped to element 0 of the image
    cgrad::wgrad_mfma<HW>(rows, co0, ci0, CI, slab_w + (size_t)blockIdx.y * ENC_CONV_P, first,
        [=](int r, int pos) {                                             // A(i = co = n, k = position)
            const float* gr = g + ((size_t)r * CO + co0 + n) * HW;
            float av[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool ok = pos + s < HW;
                av[s] = gr[ok ? pos + s : 0];
                av[s] = ok ? av[s] : 0.0f;
            }
            return make_float4(av[0], av[1], av[2], av[3]);
        },
        [=](int r, int pos, int ky, int kx) {                             // B(k = position, j = ci = n)
            const bool ok = pos < HW;
            const int pc = ok ? pos : 0, oy = pc / HOUT, ox = pc - oy * HOUT;
            const float bv = (x + ((size_t)r * CI + ci0 + n) * XW)[(2 * oy + ky) * HIN + 2 * ox + kx];
            return ok ? bv : 0.0f;
        });
}

// layer 1's weights: dW1[co][tap] = sum g1[m][co][oy][ox] o[m][2 oy + ky][2 ox + kx]; grid (32, G)
__global__ void __launch_bounds__(256) k_enc_w1(const float* __restrict__ o, const float* __restrict__ g1, float* __restrict__ slab_w, int rows, int first) {
#pragma clang fp contract(off)
    const int co = blockIdx.x;
    cgrad::wgrad_valu(rows, 961, slab_w + (size_t)blockIdx.y * ENC_CONV_P + co * 9, first, [=](int r, int i, float& c, float (&t9)[9]) {
        const int oy = i / 31, ox = i - oy * 31;
        const float* xp = o + (size_t)r * 4096 + (2 * oy) * 64 + 2 * ox;
        c = g1[((size_t)r * 32 + co) * 961 + i];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) t9[3 * ky + kx] = xp[ky * 64 + kx];
    });
}

// g [rows][CO][HOUT][HOUT] -> dx [rows][CI][HIN][HIN], gated by gate > 0 (the layer's stored input, same shape)
template <int CI, int CO, int HIN>
__global__ void __launch_bounds__(256) k_enc_dx(const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ gate,
                                                float* __restrict__ dx, int rows) {
#pragma clang fp contract(off)
    constexpr int HOUT = (HIN - 1) / 2, GW = HOUT * HOUT, NE = HOUT + 1, PT = (NE * NE + 15) / 16, PER_ROW = (CI / 16) * 4 * PT;
    static_assert(CI % 16 == 0 && CO % 4 == 0 && 2 * HOUT + 1 == HIN, "whole channel tiles, odd extent");
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW;
    int t_ = task - r * PER_ROW;
    const int pt = t_ % PT; t_ /= PT;
    const int cls = t_ & 3, ci0 = 16 * (t_ >> 2);
    const int py = cls >> 1, px = cls & 1;                       // the class holds iy = 2 vy + py, ix = 2 vx + px: ny x nx positions
    const int ny = py ? HOUT : NE, nx = px ? HOUT : NE;
    if (16 * pt >= ny * nx) return;
    const int p = 16 * pt + n;
    const bool ok = p < ny * nx;
    const int pc = ok ? p : 0, vy = pc / nx, vx = pc - vy * nx;
    const float* gr = g + (size_t)r * CO * GW;                   // B(k = co, j = position n)
    const float* wr = W + (size_t)(ci0 + n) * 9;                 // A(i = ci n, k = co): W[co][ci][tap]
    f32x4 total = (f32x4)(0.f);
#pragma unroll 1
    for (int ky = py; ky < 3; ky += 2) {
#pragma unroll 1
        for (int kx = px; kx < 3; kx += 2) {
            const int oy = vy - ((ky - py) >> 1), ox = vx - ((kx - px) >> 1);
            const bool v = ok && oy >= 0 && oy < HOUT && ox >= 0 && ox < HOUT;
            const int off = v ? oy * HOUT + ox : 0, tap = 3 * ky + kx;
            f32x4 c = (f32x4)(0.f);
#pragma unroll 4
            for (int k0 = 0; k0 < CO; k0 += 4) {
                const int k = k0 + q;
                float bv = gr[(size_t)k * GW + off];
                bv = v ? bv : 0.0f;
                c = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[(size_t)k * CI * 9 + tap], bv, c, 0, 0, 0);
            }
            total = total + c;
        }
    }
    if (!ok) return;
    const int iy = 2 * vy + py, ix = 2 * vx + px;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t idx = ((size_t)r * CI + ci0 + 4 * q + e) * HIN * HIN + iy * HIN + ix;      // D(i = 4 q + e, j = n)
        dx[idx] = gate_open(gate[idx]) ? total[e] : 0.0f;
    }
}

// ---- the gradient of mean(F_down) at the latent (compute_loss_down, torchloss.py:53-74; ps1 and omega are constants there) -------------
//   dkl_s / dmu = 2 (mu - ps1_mean) / den,  dkl_s / dlv = exp(lv) / den - 0.5,  den = 2 exp(ps1_logvar) / w
//   dkl_n / dmu = mu w,                     dkl_n / dlv = exp(lv) w / 2 - 0.5
//   g_mean = d_s + (c_s dkl_s/dmu + c_n dkl_n/dmu) / M,   g_logvar = d_s eps 0.5 exp(0.5 lv) + (c_s dkl_s/dlv + c_n dkl_n/dlv) / M
// (c_s, c_n) = beta_s (gamma, 1 - gamma) with k_fe_down's fp32 branches on gamma; eps = the injected normal, else launch_root_post's draw
// evaluated again by the same philox.h function
__global__ void __launch_bounds__(256) k_down_latent(const DownLatentArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.rows * S_DIM_FE) return;
    const int r = i / S_DIM_FE, k = i - r * S_DIM_FE;
    const float w = a.omega_in ? a.omega_in[r] : a.omega_scalar;
    const float mu = a.mean[i], lv = a.logvar[i], ds = a.d_s[i];
    const float eps = a.eps_inj ? a.eps_inj[i] : normal_elem(a.key.k0, a.key.k1, a.key.row0 + (uint32_t)r, a.key.stream, a.key.stage, k);
    const float den = (2.0f * expf(a.p1_lv[i])) / w, elv = expf(lv);
    const float dsm = (2.0f * (mu - a.p1_mean[i])) / den, dsl = elv / den - 0.5f;
    const float dnm = mu * w, dnl = (elv * w) / 2.0f - 0.5f;
    float cs, cn;
    if (a.gamma <= 0.05f) { cs = 0.0f; cn = a.beta_s; }
    else if (a.gamma >= 0.95f) { cs = a.beta_s; cn = 0.0f; }
    else { cs = a.beta_s * a.gamma; cn = a.beta_s * (1.0f - a.gamma); }
    a.g_mean[i] = ds + (cs * dsm + cn * dnm) / a.Mf;
    a.g_logvar[i] = ((ds * eps) * 0.5f) * expf(0.5f * lv) + (cs * dsl + cn * dnl) / a.Mf;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
namespace {

template <int CI, int CO, int HIN>
void conv(const float* x, const float* W, const float* bias, float* y, int rows, hipStream_t st) {
    constexpr int HOUT = (HIN - 1) / 2, per_row = (CO / 16) * ((HOUT * HOUT + 15) / 16);
    hipLaunchKernelGGL((k_enc_conv<CI, CO, HIN>), dim3((unsigned)((rows * per_row + 3) / 4)), dim3(256), 0, st, x, W, bias, y, rows);
}
template <int CI, int CO, int HIN>
void wgrad(const float* x, const float* g, float* slab_w, int rows, int G, int first, hipStream_t st) {
    hipLaunchKernelGGL((k_enc_wgrad<CI, CO, HIN>), dim3((CI / 16) * (CO / 16) / 4, G), dim3(256), 0, st, x, g, slab_w, rows, first);
}
template <int CI, int CO, int HIN>
void dgrad(const float* g, const float* W, const float* gate, float* dx, int rows, hipStream_t st) {
    constexpr int NE = (HIN + 1) / 2, per_row = (CI / 16) * 4 * ((NE * NE + 15) / 16);
    hipLaunchKernelGGL((k_enc_dx<CI, CO, HIN>), dim3((unsigned)((rows * per_row + 3) / 4)), dim3(256), 0, st, g, W, gate, dx, rows);
}
void bias(const float* g, int CO, int HW, float* slab_b, int rows, int G, int first, hipStream_t st) {
    launch_conv_bias(g, CO, HW, slab_b, rows, G, ENC_CONV_P, first, st);
}

}  // namespace

void launch_enc_train_fwd(const EncTrainArgs& a, hipStream_t st) {
    const int R = a.rows;
    const float* w = a.w;
    hipLaunchKernelGGL(k_enc_conv1, dim3((unsigned)((R * 32 * 961 + 255) / 256)), dim3(256), 0, st, a.o, w, a.y1, R);
    conv<32, 32, 31>(a.y1, w + EQ_W2, w + EQ_B2, a.y2, R, st);
    conv<32, 64, 15>(a.y2, w + EQ_W3, w + EQ_B3, a.y3, R, st);
    conv<64, 64, 7>(a.y3, w + EQ_W4, w + EQ_B4, a.y4, R, st);
    hipLaunchKernelGGL(k_ench_fwd, dim3((R + TR - 1) / TR), dim3(256), 0, st, a);
}

void launch_enc_train_bwd(const EncTrainArgs& a, hipStream_t st) {
    const int R = a.rows, G = a.GC, first = a.first;
    const float* w = a.w;
    hipLaunchKernelGGL(k_ench_bwd, dim3((R + TR - 1) / TR), dim3(256), 0, st, a);
    // layer 4
    wgrad<64, 64, 7>(a.y3, a.g4, a.cslabs + EQ_W4, R, G, first, st);
    bias(a.g4, 64, 9, a.cslabs + EQ_B4, R, G, first, st);
    dgrad<64, 64, 7>(a.g4, w + EQ_W4, a.y3, a.g3, R, st);
    // layer 3
    wgrad<32, 64, 15>(a.y2, a.g3, a.cslabs + EQ_W3, R, G, first, st);
    bias(a.g3, 64, 49, a.cslabs + EQ_B3, R, G, first, st);
    dgrad<32, 64, 15>(a.g3, w + EQ_W3, a.y2, a.g2, R, st);
    // layer 2
    wgrad<32, 32, 31>(a.y1, a.g2, a.cslabs + EQ_W2, R, G, first, st);
    bias(a.g2, 32, 225, a.cslabs + EQ_B2, R, G, first, st);
    dgrad<32, 32, 31>(a.g2, w + EQ_W2, a.y1, a.g1, R, st);
    // layer 1 (no gradient with respect to the image)
    hipLaunchKernelGGL(k_enc_w1, dim3(32, G), dim3(256), 0, st, a.o, a.g1, a.cslabs + EQ_W1, R, first);
    bias(a.g1, 32, 961, a.cslabs + EQ_B1, R, G, first, st);
}

void launch_down_latent(const DownLatentArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_down_latent, dim3((a.rows * S_DIM_FE + 255) / 256), dim3(256), 0, st, a);
}

}  // namespace efe
