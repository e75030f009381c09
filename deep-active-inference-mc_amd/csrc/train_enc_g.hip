// train_enc.hip at every admitted geometry: forward for training and backward of the encoder ModelDown.qs_net (the reference's
// src/torchmodel.py:84-104) with every size taken from the context: C = 1..3 input channels, resolution R = 32..128 in steps of 4.  With
// train_dec_head_g.hip and train_dec_g.hip: the gradient of mean(F_down) of train_model_down with respect to every parameter of ModelDown at
// C x R x R.  The mathematics is train_enc.hip's; only the channel counts (32 / 64) are template parameters, never a spatial size.
//     x0 = o [C][R][R]                          the caller's NCHW image, read directly
//     y1 = relu(Conv2d( C, 32, k3, s2)(x0))   [32][H1][H1]        H_l = (H_{l-1} - 3) / 2 + 1, H_0 = R
//     y2 = relu(Conv2d(32, 32, k3, s2)(y1))   [32][H2][H2]
//     y3 = relu(Conv2d(32, 64, k3, s2)(y2))   [64][H3][H3]
//     y4 = relu(Conv2d(64, 64, k3, s2)(y3))   [64][H4][H4]        flattened in the reference's order c H4^2 + p: K = 64 H4^2 inputs of qs_net.9
//     h1 = relu(W9 y4 + b) keep0 2,  h2 = relu(W12 h1 + b) keep1 2,  h3 = relu(W15 h2 + b) keep2 2      [256]
//     out = W18 h3 + b = (mean[10], logvar[10])
// (H1, H2, H3, H4) runs from (15, 7, 3, 1) at R = 32 to (63, 31, 15, 7) at R = 128; K = 64, 256, 576, 1 024, 1 600, 2 304, 3 136.  W comes from
// the raw device copy in parameters() order (EncGeo of kernels.h).
//
// Even extents.  At 1 x 64 x 64 every extent is odd; here they are not (84 -> 41, 20, 9, 4).  A layer whose input extent is even never reads
// the last row and column of its input.  k_encg_dx walks EVERY position of the input grid, ceil(HIN / 2) rows and columns per parity class,
// so those positions are stored: no tap reaches them, every MFMA operand of theirs is zero, and the stored value is an exact zero whatever
// the arena held.  The layer below forms its weight and bias gradient over every position of g, these zeros included.
//
// Ragged tiles (H4 = 1: one live lane of 16; H3 = 3: nine): a padding lane feeds exact zeros into both MFMA operands, its address is clamped
// to element 0 of its own image (row 0 of the group for a padding row), and it stores nothing.  Offsets are formed in size_t.
//
// Dropout: the keep mask of head layer li = 0..2 is the forward encoder's at that geometry, draw for draw: tag TAG_ENC + li, block f >> 7,
// word (f >> 5) & 3, bit f & 31, the call's row / stream / stage.  Backward gates are read off the stored activations.
//
// Kernels (one row group of at most DecTailGeo::rows_per_pass() rows, 64 while B <= 16, else 32, per launch):
//   k_encg_conv1   : layer 1 on the VALU, one thread per output, a loop over the C input channels.
//   k_encg_conv<CI, CO>   : layers 2..4 on v_mfma_f32_16x16x4_f32: one wave = 16 output channels x 16 consecutive output positions.
//   k_enchg_fc0    : partial sums of W9 y4 over S = ceil(K / 256) segments of 256 inputs; one wave = 16 features of one segment (its
//                    16 x 256 weights stay in registers) x every 16-row tile.
//   k_enchg_join   : joins the S partials of a (row, feature), adds the bias, ReLU and mask: h1.  One workgroup per row.
//   k_enchg_fwd    : layers .12 / .15 / .18 over one 16-row tile, activations in LDS (49 920 B): h2, h3, mean, logvar.
//   k_enchg_small  : layers .18 / .15 / .12 backward over one 16-row tile from the upstream pair, train_mlp.h's passes (the 20-wide last
//                    layer BOUND); ends in g_0 = dL / da of qs_net.9, stored.  LDS 35 584 B.
//   k_enchg_w9grad : dW9, db9; one wave owns 16 features x 64 inputs (K = the rows), written / added into the caller's gradient.
//   k_enchg_dy4    : g4 = (g_0 W9) [y4 > 0]: one contract<8, 16> over the 256 features per element; one wave = 16 inputs x every tile.
//   k_encg_wgrad<CI, CO>  : train_conv.h's wgrad_mfma_rt, layers 2..4.   k_encg_w1 : the 288 C weights of layer 1 (wgrad_valu), one
//                    workgroup per (co, ci, slab).   k_conv_bias (train_dec.hip).   k_encg_dx<CI, CO> : the data gradient, per parity class.
//   k_slab_sum (train.hip).
//
// Forward order: conv1 one 9-term fma chain (ky, kx ascending) per input channel, the channels added in ascending order, + bias.  Layers
// 2..4: train_enc.hip's (three chains per kernel row).  qs_net.9: segment j = inputs 256 j .. 256 j + 255 = tree<8> of eight chains over
// the 16-input chunks c = 0..15 (chunk c on accumulator c & 7); a chunk behind K (the last segment of K = 576, 1 600, 3 136 holds 4
// chunks; K = 64 has ONE segment of 4 chunks) feeds exact zeros into both operands, address clamped to the segment's chunk 0: at K = 64
// accumulators 4..7 stay + 0 and tree<8> adds them.  The segments are joined as in train_dec_head_g.hip: sequential sums of runs of eight
// consecutive segments ascending, the last run shorter, the runs added ascending; then + bias.  Layers .12 .. .18: contract<8, 16>.
// The data gradient of the convolutions: per tap in (ky, kx) ascending order one chain over the output channels, sum = sum + tap.
//
// Reduction-order contract of the parameter gradient (a function of the geometry and M alone, no float atomics; every (element, slab) has
// ONE owning thread; two identical calls give identical bits):
//   rows     : row group g = rows P g .. P g + P - 1, P = rows_per_pass(); 16-row tile t = rows 16 t .. 16 t + 15 of the CALL; rows >= M
//              contribute exact zeros.
//   convs    : GC = min(M, 32) slabs of 64 704 + 288 C floats; row m belongs to slab m mod GC.  Chunk, image, group and slab order:
//              train_conv.h; the last chunk of an image is ragged.
//   dW9/db9  : per element and group, the tiles ascending: chunk = one 16-term MFMA chain over the tile's rows (db: a sequential sum),
//              group = ((chunk_0 + chunk_1) + ...); gradient = ((group_0 + group_1) + ...) ascending, in place.
//   .12-.18  : GH = min(ceil(M / 16), 4) slabs of ENC_SMALL_P = 136 724 floats; tile t of the call adds its 16-term chain (db: sequential
//              sum) to slab t mod 4, tiles ascending (the first four tiles write); gradient = ((slab_0 + slab_1) + slab_2) + slab_3.
// The per-row outputs (mean, logvar, y1..y4, h1..h3) depend on that row and its global row id only.  Equal bits with efe_enc_grad at
// 1 x 64 x 64 are not promised (the join of qs_net.9 and the head's slab rule differ).
#include "train_mlp.h"
#include "train_conv.h"

namespace efe {

using namespace mlp;

namespace {

constexpr int HLD = 256 + 4;       // LDS row stride of a 256-wide activation
constexpr int GLD = 32 + 4;        // ... of the upstream tile (mean | logvar, zero from column 20)

// a [16][256] activation tile of the group into LDS, zero beyond the group's rows; thread = column
__device__ __forceinline__ void load_tile256(float* dst, const float* src, int r0, int rows, int tid) {
#pragma unroll 4
    for (int r = 0; r < TR; ++r) dst[r * HLD + tid] = r0 + r < rows ? src[(size_t)(r0 + r) * 256 + tid] : 0.0f;
}

struct EncPos { int oy, ox; bool in; };       // a position of an output grid: row, column, and whether it is one (< HW)

}  // namespace

// ---- forward -----------------------------------------------------------------------------------------------------------------
// layer 1: o [rows][C][R][R] -> y1 [rows][32][H1][H1]; one thread per output
__global__ void __launch_bounds__(256) k_encg_conv1(const float* __restrict__ o, const float* __restrict__ w, const float* __restrict__ bias,
                                                    float* __restrict__ y1, int rows, int C, int R, int H1) {
#pragma clang fp contract(off)
    const int HW = H1 * H1, RR = R * R;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * 32 * HW) return;
    const int r = (int)(i / (size_t)(32 * HW)), t = (int)(i - (size_t)r * (32 * HW)), co = t / HW, pos = t - co * HW, oy = pos / H1, ox = pos - oy * H1;
    const float* x = o + (size_t)r * C * RR + (2 * oy) * R + 2 * ox;          // (last pixel read: row and column 2 H1)
    const float* wp = w + (size_t)co * C * 9;
    float total = 0.0f;
    for (int ci = 0; ci < C; ++ci) {
        float c = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) c = fmaf(x[(size_t)ci * RR + ky * R + kx], wp[ci * 9 + 3 * ky + kx], c);
        total = ci == 0 ? c : total + c;
    }
    y1[i] = relu_nan(total + bias[co]);
}

// layers 2..4: x [rows][CI][HIN][HIN] -> y = relu(conv + bias) [rows][CO][HOUT][HOUT], HOUT = (HIN - 3) / 2 + 1
template <int CI, int CO>
__global__ void __launch_bounds__(256) k_encg_conv(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ y, int rows, int HIN, int HOUT) {
#pragma clang fp contract(off)
    static_assert(CI % 4 == 0 && CO % 16 == 0, "whole channel tiles");
    const int HW = HOUT * HOUT, XW = HIN * HIN, PT = (HW + 15) / 16, PER_ROW = (CO / 16) * PT;
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW, t_ = task - r * PER_ROW, pt = t_ % PT, co0 = 16 * (t_ / PT);
    const int pos = 16 * pt + n;
    const bool ok = pos < HW;
    const int pc = ok ? pos : 0, oy = pc / HOUT, ox = pc - oy * HOUT;
    const float* xr = x + (size_t)r * CI * XW + (2 * oy) * HIN + 2 * ox;              // B(k = ci, j = position n)
    const float* wr = W + (size_t)(co0 + n) * CI * 9;                                 // A(i = co n, k = ci)
    f32x4 total = (f32x4)(0.f);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        f32x4 c[3] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll 2
        for (int k0 = 0; k0 < CI; k0 += 4) {
            const int k = k0 + q;
            const float* xp = xr + (size_t)k * XW + ky * HIN;
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

// grid = S segments x 4: wave = 16 features f0 .. f0 + 15 of one segment of 256 inputs; part[seg][row][f] = sum_{k in seg} W9[f][k] y4[row][k].
// A chunk of 16 inputs lies wholly inside K or wholly behind it (K is a multiple of 64)
__global__ void __launch_bounds__(256) k_enchg_fc0(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int seg = blockIdx.x >> 2;
    const int f0 = 16 * __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 3) * 4 + (int)(threadIdx.x >> 6));
    const int K = a.geo.K(), ks = seg * 256;
    const int nc = min(16, (K - ks) >> 4);                                                              // chunks of this segment inside K: 16, or 4
    const float* Wr = a.w + a.geo.w9() + (size_t)(f0 + n) * K + ks + 4 * q;
    float4 av[16];                                                                                      // A(i = feature, k): W9[f0 + n][ks + 16 c + 4 q + s]
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const bool in = c < nc;
        const float4 v = *reinterpret_cast<const float4*>(Wr + (in ? 16 * c : 0));
        av[c] = in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        const int row = r0 + n;
        const bool ok = row < a.rows;
        const float* xp = a.y4 + (size_t)(ok ? row : 0) * K + ks + 4 * q;
        const f32x4 sum = contract<8, 16>([&](int c) { return av[c]; }, [&](int c) {                    // D(i = feature 4 q + e, j = row n)
            const bool in = ok && c < nc;
            float4 bv = *reinterpret_cast<const float4*>(xp + (c < nc ? 16 * c : 0));                   // B(k = input, j = row)
            if (!in) bv = make_float4(0.f, 0.f, 0.f, 0.f);
            return bv;
        });
        if (ok) *reinterpret_cast<float4*>(a.part + ((size_t)seg * a.rows + row) * 256 + f0 + 4 * q) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
}

// grid = rows: thread = feature f of one row.  h1[row][f] = relu(join of the S segment partials + bias) keep 2.  Eight loads of a run are in
// flight at once; a segment >= S of the last run reads the run's first segment and is not added
__global__ void __launch_bounds__(256) k_enchg_join(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, f = threadIdx.x, S = a.geo.segs();
    const float* pp = a.part + (size_t)row * 256 + f;
    const size_t ss = (size_t)a.rows * 256;
    float sum = 0.0f;
#pragma unroll 1
    for (int j0 = 0; j0 < S; j0 += 8) {                  // run = segments j0 .. j0 + 7 (the last run shorter), a sequential sum
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = pp[(size_t)(j0 + i < S ? j0 + i : j0) * ss];
        float sm = v[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) sm = j0 + i < S ? sm + v[i] : sm;
        sum = j0 == 0 ? sm : sum + sm;                   // the runs in ascending order
    }
    const uint32_t word = pick(mask_block(a.key, TAG_ENC, (uint32_t)(f >> 7), (uint32_t)row), (f >> 5) & 3);
    a.h1[(size_t)row * 256 + f] = relu_drop(sum + a.w[a.geo.b9() + f], true, true, word, f & 31);
}

// layers .12 / .15 / .18: grid = ceil(rows / 16); H[0] = h1 as k_enchg_join stored it
__global__ void __launch_bounds__(256) k_enchg_fwd(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float H[3 * TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, row = r0 + n;
    const bool rok = row < a.rows;
    const gfloat* ws = (const gfloat*)a.w + a.geo.small();
    load_tile256(H, a.h1, r0, a.rows, tid);
    __syncthreads();
#pragma unroll 1
    for (int l = 1; l < 4; ++l) {
        const gfloat* W = ws + (l == 1 ? EQS_W12 : l == 2 ? EQS_W15 : EQS_W18);
        const gfloat* B = ws + (l == 1 ? EQS_B12 : l == 2 ? EQS_B15 : EQS_B18);
        const int O = l == 3 ? 20 : 256, NT = l == 3 ? 2 : 16;
        float* hl = l == 1 ? a.h2 : a.h3;
#pragma unroll 1
        for (int t = w; t < NT; t += 4) {
            const int f0 = 16 * t;
            const float* x = H + (l - 1) * TR * HLD + n * HLD + 4 * q;       // K = 256; the last layer's features 20..31 feed zeros, read from row 0
            const bool fin = f0 + n < O;
            const float4* Wp = reinterpret_cast<const float4*>((const float*)W + (size_t)(fin ? f0 + n : 0) * 256 + 4 * q);
            const f32x4 sum = contract<8, 16>([&](int c) {
                float4 av = Wp[4 * c];
                if (!fin) av = make_float4(0.f, 0.f, 0.f, 0.f);
                return av;
            }, [&](int c) { return *reinterpret_cast<const float4*>(x + 16 * c); });
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
// layers .18 / .15 / .12 over one 16-row tile; slab = the tile's index in the CALL mod ENC_HEAD_SLABS (a.tile0 + blockIdx.x), written by the
// call's first four tiles, added to by the later ones.  grid = ceil(rows / 16)
// LDS: G3 = g_3 (upstream) | A = x_3 = h3, then g_2 | U = x_2 = h2, then g_1; A = x_1 = h1, then g_0 -> a.g0
__global__ void __launch_bounds__(256) k_enchg_small(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float G3[TR * GLD];
    __shared__ __attribute__((aligned(16))) float A[TR * HLD];
    __shared__ __attribute__((aligned(16))) float U[TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, gt = a.tile0 + (int)blockIdx.x;
    const bool first = gt < ENC_HEAD_SLABS;
    const gfloat* wt = (const gfloat*)a.w + a.geo.small();
    gfloat* slab = (gfloat*)a.hslabs + (size_t)(gt % ENC_HEAD_SLABS) * ENC_SMALL_P;
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
    // qs_net.18 (20 outputs in a 32-wide tile, no gate on its output)
    dw_pass(G3, GLD, A, HLD, 20, 256, slab + EQS_W18, first, w, n, q);
    db_pass(G3, GLD, 20, slab + EQS_B18, first, tid);
    __syncthreads();                                                            // dW has consumed x: it may now be overwritten
    dprev_pass<8, 2, true>(G3, GLD, A, HLD, wt + EQS_W18, 256, 2.0f, true, w, n, q, 20);
    __syncthreads();
    // qs_net.15
    dw_pass(A, HLD, U, HLD, 256, 256, slab + EQS_W15, first, w, n, q);
    db_pass(A, HLD, 256, slab + EQS_B15, first, tid);
    __syncthreads();
    dprev_pass<8, 16>(A, HLD, U, HLD, wt + EQS_W15, 256, 2.0f, true, w, n, q);
    __syncthreads();
    load_tile256(A, a.h1, r0, a.rows, tid);
    __syncthreads();
    // qs_net.12
    dw_pass(U, HLD, A, HLD, 256, 256, slab + EQS_W12, first, w, n, q);
    db_pass(U, HLD, 256, slab + EQS_B12, first, tid);
    __syncthreads();
    dprev_pass<8, 16>(U, HLD, A, HLD, wt + EQS_W12, 256, 2.0f, true, w, n, q);
    __syncthreads();
#pragma unroll 4
    for (int r = 0; r < TR; ++r)
        if (r0 + r < a.rows) a.g0[(size_t)(r0 + r) * 256 + tid] = A[r * HLD + tid];
}

// grid = K / 16 workgroups: wave = 16 features x 64 inputs of dW9 (and, for the first 64 inputs, the 16 features of db9)
__global__ void __launch_bounds__(256) k_enchg_w9grad(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int K = a.geo.K(), KB = K >> 6;
    const int f0 = 16 * (wv / KB), kb = 64 * (wv % KB);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4)(0.f);
    float bacc = 0.0f;
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        f32x4 ch[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ch[t] = (f32x4)(0.f);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r0 + 4 * s + q;
            const bool ok = row < a.rows;
            const size_t rr = ok ? row : 0;
            float av = a.g0[rr * 256 + f0 + n];                                                          // A(i = feature, k = row)
            av = ok ? av : 0.0f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float bv = a.y4[rr * K + kb + 16 * t + n];                                               // B(k = row, j = input)
                bv = ok ? bv : 0.0f;
                ch[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, ch[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = acc[t] + ch[t];
        float bc = 0.0f;                                                                                 // db: the tile's rows in ascending order
#pragma unroll 4
        for (int j = 0; j < TR; ++j) {
            const bool ok = r0 + j < a.rows;
            const float v = a.g0[(size_t)(ok ? r0 + j : 0) * 256 + f0 + n];
            bc = bc + (ok ? v : 0.0f);
        }
        bacc = bacc + bc;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float* d = a.grad + a.geo.w9() + (size_t)(f0 + 4 * q + e) * K + kb + 16 * t + n;             // D(i = 4 q + e, j = n)
            *d = a.first ? acc[t][e] : *d + acc[t][e];
        }
    if (kb == 0 && q == 0) {
        float* d = a.grad + a.geo.b9() + f0 + n;
        *d = a.first ? bacc : *d + bacc;
    }
}

// grid = K / 64 workgroups: wave = 16 inputs k0 .. k0 + 15 x every 16-row tile; g4[row][k] = (sum_f g_0[row][f] W9[f][k]) [y4[row][k] > 0]
__global__ void __launch_bounds__(256) k_enchg_dy4(const EncTrainGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int k0 = 16 * __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const size_t K = (size_t)a.geo.K();
    const float* Wc = a.w + a.geo.w9() + (size_t)(4 * q) * K + k0 + n;
    float4 av[16];                                                                                      // A(i = input, k = feature): W9[16 c + 4 q + s][k0 + n]
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const size_t o = (size_t)(16 * c) * K;
        av[c] = make_float4(Wc[o], Wc[o + K], Wc[o + 2 * K], Wc[o + 3 * K]);
    }
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        const int row = r0 + n;
        const bool ok = row < a.rows;
        const float* gp = a.g0 + (size_t)(ok ? row : 0) * 256 + 4 * q;
        const f32x4 sum = contract<8, 16>([&](int c) { return av[c]; }, [&](int c) {                    // D(i = input 4 q + e, j = row n)
            float4 bv = *reinterpret_cast<const float4*>(gp + 16 * c);                                  // B(k = feature, j = row)
            if (!ok) bv = make_float4(0.f, 0.f, 0.f, 0.f);
            return bv;
        });
        if (ok) {
            const size_t idx = (size_t)row * K + k0 + 4 * q;
            const float4 y = *reinterpret_cast<const float4*>(a.y4 + idx);
            *reinterpret_cast<float4*>(a.g4 + idx) = make_float4(gate_open(y.x) ? sum[0] : 0.0f, gate_open(y.y) ? sum[1] : 0.0f,
                                                                 gate_open(y.z) ? sum[2] : 0.0f, gate_open(y.w) ? sum[3] : 0.0f);
        }
    }
}

// x [rows][CI][HIN][HIN], g [rows][CO][HOUT][HOUT] -> slab[(co CI + ci) 9 + tap]; grid ((CO / 16) (CI / 16) / 4, G)
// rcp = ceil(2^32 / HOUT): pos / HOUT = umulhi(pos, rcp), exact for every pos < 2^25 at HOUT <= 128; HOUT = 1: rcp = 0 and pos = 0 alone
template <int CI, int CO>
__global__ void __launch_bounds__(256) k_encg_wgrad(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ slab_w,
                                                    int rows, int P, int first, int HIN, int HOUT, unsigned rcp) {
#pragma clang fp contract(off)
    static_assert((CI / 16) * (CO / 16) % 4 == 0, "whole workgroups");
    const int HW = HOUT * HOUT, XW = HIN * HIN;
    const int n = threadIdx.x & 15;
    const int pair = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int co0 = 16 * (pair / (CI / 16)), ci0 = 16 * (pair % (CI / 16));
    // a position >= HW of the ragged last chunk: zero into both operands, the address clamped to element 0 of the image
    cgrad::wgrad_mfma_rt(HW, rows, co0, ci0, CI, slab_w + (size_t)blockIdx.y * P, first,
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
        [=](int r, EncPos at, int ky, int kx) {                           // B(k = position, j = ci = n)
            const float bv = (x + ((size_t)r * CI + ci0 + n) * XW)[at.in ? (2 * at.oy + ky) * HIN + 2 * at.ox + kx : 0];
            return at.in ? bv : 0.0f;
        },
        [=](int pos) {
            EncPos at;
            at.in = pos < HW;
            const int pc = at.in ? pos : 0;
            at.oy = (int)__umulhi((unsigned)pc, rcp);
            at.ox = pc - at.oy * HOUT;
            return at;
        });
}

// layer 1's weights: dW1[co][ci][tap] = sum g1[m][co][oy][ox] o[m][ci][2 oy + ky][2 ox + kx]; grid (32 C, G), blockIdx.x = co C + ci
__global__ void __launch_bounds__(256) k_encg_w1(const float* __restrict__ o, const float* __restrict__ g1, float* __restrict__ slab_w, int rows,
                                                 int P, int first, int C, int R, int H1) {
#pragma clang fp contract(off)
    const int co = blockIdx.x / C, ci = blockIdx.x - co * C, HW = H1 * H1, RR = R * R;
    cgrad::wgrad_valu(rows, HW, slab_w + (size_t)blockIdx.y * P + blockIdx.x * 9, first, [=](int r, int i, float& c, float (&t9)[9]) {
        const int oy = i / H1, ox = i - oy * H1;
        const float* xp = o + ((size_t)r * C + ci) * RR + (2 * oy) * R + 2 * ox;
        c = g1[((size_t)r * 32 + co) * HW + i];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) t9[3 * ky + kx] = xp[ky * R + kx];
    });
}

// g [rows][CO][HOUT][HOUT] -> dx [rows][CI][HIN][HIN], gated by gate > 0 (the layer's stored input, same shape).  Class (py, px) holds the
// positions iy = 2 vy + py < HIN, ix = 2 vx + px < HIN: ceil((HIN - py) / 2) x ceil((HIN - px) / 2) of them, EVERY position of the grid.
// At an even HIN the last row and column (class py = 1 / px = 1, vy = HOUT / vx = HOUT) are reached by no tap: stored as exact zeros
template <int CI, int CO>
__global__ void __launch_bounds__(256) k_encg_dx(const float* __restrict__ g, const float* __restrict__ W, const float* __restrict__ gate,
                                                 float* __restrict__ dx, int rows, int HIN, int HOUT) {
#pragma clang fp contract(off)
    static_assert(CI % 16 == 0 && CO % 4 == 0, "whole channel tiles");
    const int GW = HOUT * HOUT, XW = HIN * HIN, NE = (HIN + 1) / 2, PT = (NE * NE + 15) / 16, PER_ROW = (CI / 16) * 4 * PT;
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW;
    int t_ = task - r * PER_ROW;
    const int pt = t_ % PT; t_ /= PT;
    const int cls = t_ & 3, ci0 = 16 * (t_ >> 2);
    const int py = cls >> 1, px = cls & 1;
    const int ny = (HIN - py + 1) / 2, nx = (HIN - px + 1) / 2;
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
        const size_t idx = ((size_t)r * CI + ci0 + 4 * q + e) * XW + iy * HIN + ix;               // D(i = 4 q + e, j = n)
        dx[idx] = gate_open(gate[idx]) ? total[e] : 0.0f;
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
namespace {

template <int CI, int CO>
void conv(const float* x, const float* W, const float* bias, float* y, int rows, int HIN, int HOUT, hipStream_t st) {
    const int per_row = (CO / 16) * ((HOUT * HOUT + 15) / 16);
    hipLaunchKernelGGL((k_encg_conv<CI, CO>), dim3((unsigned)((rows * per_row + 3) / 4)), dim3(256), 0, st, x, W, bias, y, rows, HIN, HOUT);
}
template <int CI, int CO>
void wgrad(const float* x, const float* g, float* slab_w, int rows, int G, int P, int first, int HIN, int HOUT, hipStream_t st) {
    const unsigned rcp = HOUT == 1 ? 0u : (unsigned)((((uint64_t)1 << 32) + (uint64_t)HOUT - 1) / (uint64_t)HOUT);
    hipLaunchKernelGGL((k_encg_wgrad<CI, CO>), dim3((CI / 16) * (CO / 16) / 4, G), dim3(256), 0, st, x, g, slab_w, rows, P, first, HIN, HOUT, rcp);
}
template <int CI, int CO>
void dgrad(const float* g, const float* W, const float* gate, float* dx, int rows, int HIN, int HOUT, hipStream_t st) {
    const int NE = (HIN + 1) / 2, per_row = (CI / 16) * 4 * ((NE * NE + 15) / 16);
    hipLaunchKernelGGL((k_encg_dx<CI, CO>), dim3((unsigned)((rows * per_row + 3) / 4)), dim3(256), 0, st, g, W, gate, dx, rows, HIN, HOUT);
}

}  // namespace

void launch_enc_train_g_fwd(const EncTrainGArgs& a, hipStream_t st) {
    const EncGeo& geo = a.geo;
    const int N = a.rows, H1 = geo.H1(), H2 = geo.H2(), H3 = geo.H3(), H4 = geo.H4();
    const float* w = a.w;
    hipLaunchKernelGGL(k_encg_conv1, dim3((unsigned)(((size_t)N * 32 * H1 * H1 + 255) / 256)), dim3(256), 0, st, a.o, w + geo.w1(), w + geo.b1(), a.y1, N,
                       geo.C, geo.R, H1);
    conv<32, 32>(a.y1, w + geo.w2(), w + geo.b2(), a.y2, N, H1, H2, st);
    conv<32, 64>(a.y2, w + geo.w3(), w + geo.b3(), a.y3, N, H2, H3, st);
    conv<64, 64>(a.y3, w + geo.w4(), w + geo.b4(), a.y4, N, H3, H4, st);
    hipLaunchKernelGGL(k_enchg_fc0, dim3(geo.segs() * 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_enchg_join, dim3(N), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_enchg_fwd, dim3((N + TR - 1) / TR), dim3(256), 0, st, a);
}

void launch_enc_train_g_bwd(const EncTrainGArgs& a, hipStream_t st) {
    const EncGeo& geo = a.geo;
    const int N = a.rows, G = a.GC, first = a.first, P = geo.conv_P(), H1 = geo.H1(), H2 = geo.H2(), H3 = geo.H3(), H4 = geo.H4();
    const float* w = a.w;
    hipLaunchKernelGGL(k_enchg_small, dim3((N + TR - 1) / TR), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_enchg_w9grad, dim3(geo.K() / 16), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_enchg_dy4, dim3(geo.K() / 64), dim3(256), 0, st, a);
    // layer 4
    wgrad<64, 64>(a.y3, a.g4, a.cslabs + geo.w4(), N, G, P, first, H3, H4, st);
    launch_conv_bias(a.g4, 64, H4 * H4, a.cslabs + geo.b4(), N, G, P, first, st);
    dgrad<64, 64>(a.g4, w + geo.w4(), a.y3, a.g3, N, H3, H4, st);
    // layer 3
    wgrad<32, 64>(a.y2, a.g3, a.cslabs + geo.w3(), N, G, P, first, H2, H3, st);
    launch_conv_bias(a.g3, 64, H3 * H3, a.cslabs + geo.b3(), N, G, P, first, st);
    dgrad<32, 64>(a.g3, w + geo.w3(), a.y2, a.g2, N, H2, H3, st);
    // layer 2
    wgrad<32, 32>(a.y1, a.g2, a.cslabs + geo.w2(), N, G, P, first, H1, H2, st);
    launch_conv_bias(a.g2, 32, H2 * H2, a.cslabs + geo.b2(), N, G, P, first, st);
    dgrad<32, 32>(a.g2, w + geo.w2(), a.y1, a.g1, N, H1, H2, st);
    // layer 1 (no gradient with respect to the image)
    hipLaunchKernelGGL(k_encg_w1, dim3(32 * geo.C, G), dim3(256), 0, st, a.o, a.g1, a.cslabs + geo.w1(), N, P, first, geo.C, geo.R, H1);
    launch_conv_bias(a.g1, 32, H1 * H1, a.cslabs + geo.b1(), N, G, P, first, st);
}

}  // namespace efe
