// Forward for training and backward of the decoder's dense head, ModelDown.po_net[0:12] (/root/reference/src/torchmodel.py:107-118), at
// the Dynamic-dSprites geometry 1 x 64 x 64: with the ConvTranspose2d tail of train_dec.hip the gradient of the reconstruction term of
// train_model_down (torchloss.py:90-98) with respect to every decoder parameter and to s.
//     a_l = W_l x_l + b_l,   x_{l+1} = relu(a_l) * keep_l * 2      l = 0..3:  s[10] -> 256 -> 256 -> 256 -> 16384 = h4 (Unflatten's input)
//     g_3 = d_h4 * 2 [h4 > 0],   dW_l = g_l^T x_l,   db_l = sum_r g_l,   g_{l-1} = (g_l W_l) * 2 [x_l > 0],   d_s = g_0 W_0
// W_l [out][in] row-major comes from the raw device copy of the parameters (flat, parameters() order, DH_* offsets of kernels.h).  h4 is
// stored in the reference's order c 256 + p, which launch_dec_tail_group consumes.
//
// Dropout: the keep mask of layer li is the forward decoder's (k_head / k_fc4), draw for draw: tag TAG_DEC + li, block f >> 7, word
// (f >> 5) & 3, bit f & 31, the call's row / stream / stage.  Layer 3's mask is indexed by the engine's NHWC feature f' = p 64 + c of the
// reference feature c 256 + p (k_fc4 emits NHWC).
//
// Kernels (one row group of at most DEC_TAIL_ROWS = 64 rows per launch):
//   k_dech_fwd   : layers 0..2, one workgroup per 16-row tile, activations in LDS and stored to h1..h3.
//   k_dech_fc4   : layer 3; one wave = 16 features (its 16 x 256 weights stay in registers) x every 16-row tile of the group.
//   k_dech_gate  : g_3 = d_h4 * 2 [h4 > 0], in place.
//   k_dech_w4grad: dW_3, db_3; one wave owns 16 features x 128 inputs (K = the rows), result written / added into the caller's gradient.
//   k_dech_dh3   : partial sums of g_3 W_3 over DEC_HEAD_SEGS = 64 segments of 256 features; one wave = 16 inputs of one segment.
//   k_dech_small : joins the partials (+ gate) and runs layers 2, 1, 0 backward over one 16-row tile in LDS; slab = tile of the group.
//   k_slab_sum (train.hip) : gradient of layers 0..2 = ascending sum of the slabs.
//
// Chains: train_mlp.h's with EIGHT accumulators over K = 256 features (32 terms per accumulator), tree<8> = ((a0 + a1) + (a2 + a3)) +
// ((a4 + a5) + (a6 + a7)).  Layer 0 (K = 10) is one chunk.  The forward order is not k_head's or k_fc4's: po1 agrees with efe_decoder to
// rounding, not bit for bit.
//
// Reduction order of the head's gradient, on top of train_mlp.h's tile, slab and gate rules (every element has ONE owning thread):
//   rows     : row group g = rows 64 g .. 64 g + 63, 16-row tile t = rows 16 t .. 16 t + 15; rows >= M contribute exact zeros.
//   dW_3/db_3: per element and group, the tiles ascending: chunk = one 16-term MFMA chain over the tile's rows (db: a sequential sum),
//              group = ((chunk_0 + chunk_1) + chunk_2) + chunk_3; gradient = ((group_0 + group_1) + ...) ascending, in place.
//   d_h3     : per row (no cross-row term): segment = tree<8> of eight 32-term chains; the 64 segments joined as tree<8> of eight sequential
//              sums of eight consecutive segments.
//   layers 0..2: G = min(ceil(M / 16), DEC_HEAD_SLABS = 4) slabs of 134 400 floats; tile t adds its 16-term chain (db: sequential sum) to
//              slab t mod 4, tiles ascending; gradient = ((slab_0 + slab_1) + slab_2) + slab_3.
// Two identical calls give identical bits; h1..h4, d_s (and through the tail po1, nlogpo1) of a row depend on that row and its global
// row id only.
#include "train_mlp.h"

namespace efe {

using namespace mlp;

namespace {

constexpr int HLD = 256 + 4;       // LDS row stride of a 256-wide activation
constexpr int SLD = 16 + 4;        // ... of the input tile s (10 columns, zero up to 16)

}  // namespace

// grid = ceil(rows / 16)
__global__ void __launch_bounds__(256) k_dech_fwd(const DecHeadArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float X0[TR * SLD];
    __shared__ __attribute__((aligned(16))) float H[3 * TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, row = r0 + n;
    {
        const int r = tid >> 4, c = tid & 15;
        X0[r * SLD + c] = (r0 + r < a.rows && c < 10) ? a.s[(size_t)(r0 + r) * 10 + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
        const gfloat* W = (const gfloat*)a.w + (l == 0 ? DH_W0 : l == 1 ? DH_W1 : DH_W2);
        const gfloat* B = (const gfloat*)a.w + (l == 0 ? DH_B0 : l == 1 ? DH_B1 : DH_B2);
        float* hl = l == 0 ? a.h1 : l == 1 ? a.h2 : a.h3;
        const float* x = (l == 0 ? X0 + n * SLD : H + (l - 1) * TR * HLD + n * HLD) + 4 * q;
        float* y = H + l * TR * HLD + n * HLD;
#pragma unroll 1
        for (int t = 4 * w; t < 4 * w + 4; ++t) {
            const int f0 = 16 * t;
            const auto ldb = [&](int c) { return *reinterpret_cast<const float4*>(x + 16 * c); };     // B(k, j = row): x[n][16 c + 4 q + s]
            f32x4 sum;
            if (l == 0) {                     // K = 10: one chunk, zero beyond the layer's width
                sum = contract<8, 1>([&](int) {                                                     // A(i = feature, k): W[f0 + n][4 q + s]
                    float av[4];
#pragma unroll
                    for (int s = 0; s < 4; ++s) av[s] = 4 * q + s < 10 ? W[(size_t)(f0 + n) * 10 + 4 * q + s] : 0.0f;
                    return make_float4(av[0], av[1], av[2], av[3]);
                }, ldb);
            } else {
                const float4* Wp = reinterpret_cast<const float4*>((const float*)W + (size_t)(f0 + n) * 256 + 4 * q);
                sum = contract<8, 16>([&](int c) { return Wp[4 * c]; }, ldb);                       // W[f0 + n][16 c + 4 q + s]
            }
            const uint32_t word = mask_word(mask_block(a.key, TAG_DEC + (uint32_t)l, (uint32_t)(f0 >> 7), (uint32_t)row), f0);
            const float4 out = fwd_epilogue(sum, B, f0, q, 256, true, true, word);                      // D(i = 4 q + e, j = n)
            *reinterpret_cast<float4*>(y + f0 + 4 * q) = out;
            if (row < a.rows) *reinterpret_cast<float4*>(hl + (size_t)row * 256 + f0 + 4 * q) = out;
        }
        __syncthreads();
    }
}

// grid = 256 workgroups: wave = 16 consecutive reference features f = c 256 + p (one channel c, pixels p0 .. p0 + 15)
__global__ void __launch_bounds__(256) k_dech_fc4(const DecHeadArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int f0 = 16 * __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const float4* Wp = reinterpret_cast<const float4*>(a.w + DH_W3 + (size_t)(f0 + n) * 256 + 4 * q);
    float4 av[16];                                                                                      // A(i = feature, k): W[f0 + n][16 c + 4 q + s]
#pragma unroll
    for (int c = 0; c < 16; ++c) av[c] = Wp[4 * c];
    const float4 bias = *reinterpret_cast<const float4*>(a.w + DH_B3 + f0 + 4 * q);
    // the mask bit of feature c 256 + p is bit f' & 31 of word (f' >> 5) & 3 of block f' >> 7, f' = p 64 + c: for this lane's pixels
    // p0 + 4 q + e that is blocks pb, pb, pb + 1, pb + 1 (pb = (p0 + 4 q) / 2), words wc, wc + 2, wc, wc + 2 (wc = c / 32), bit c % 32
    const int ch = f0 >> 8, p0 = f0 & 255;
    const uint32_t pb = (uint32_t)((p0 + 4 * q) >> 1);
    const int wc = ch >> 5, bit = ch & 31;
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        const int row = r0 + n;
        const bool ok = row < a.rows;
        const float* xp = a.h3 + (size_t)(ok ? row : 0) * 256 + 4 * q;
        const f32x4 sum = contract<8, 16>([&](int c) { return av[c]; }, [&](int c) {
            float4 bv = *reinterpret_cast<const float4*>(xp + 16 * c);                                  // B(k, j = row): h3[row][16 c + 4 q + s]
            if (!ok) bv = make_float4(0.f, 0.f, 0.f, 0.f);
            return bv;
        });
        const uint4 ra = mask_block(a.key, TAG_DEC + 3u, pb, (uint32_t)row), rb = mask_block(a.key, TAG_DEC + 3u, pb + 1u, (uint32_t)row);
        const uint32_t keep[4] = {pick(ra, wc), pick(ra, wc + 2), pick(rb, wc), pick(rb, wc + 2)};
        const float b4[4] = {bias.x, bias.y, bias.z, bias.w};
        float4 out;
        float* o4 = &out.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = relu_drop(sum[e] + b4[e], true, true, keep[e], bit);
        if (ok) *reinterpret_cast<float4*>(a.h4 + (size_t)row * 16384 + f0 + 4 * q) = out;
    }
}

// g[i] = h4[i] > 0 ? 2 g[i] : 0; one thread per four elements
__global__ void __launch_bounds__(256) k_dech_gate(const float* __restrict__ h4, float* __restrict__ g, int n4) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 h = reinterpret_cast<const float4*>(h4)[i];
    float4 v = reinterpret_cast<float4*>(g)[i];
    v.x = gated(h.x, 2.0f * v.x, true, true);
    v.y = gated(h.y, 2.0f * v.y, true, true);
    v.z = gated(h.z, 2.0f * v.z, true, true);
    v.w = gated(h.w, 2.0f * v.w, true, true);
    reinterpret_cast<float4*>(g)[i] = v;
}

// grid = 512 workgroups: wave = 16 features x 128 inputs of dW_3 (and, in the first half, the 16 features of db_3)
__global__ void __launch_bounds__(256) k_dech_w4grad(const DecHeadArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int f0 = 16 * (wv >> 1), kb = 128 * (wv & 1);
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = (f32x4)(0.f);
    float bacc = 0.0f;
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        f32x4 ch[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) ch[t] = (f32x4)(0.f);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int row = r0 + 4 * s + q;
            const bool ok = row < a.rows;
            const size_t rr = ok ? row : 0;
            float av = a.g4[rr * 16384 + f0 + n];                                                        // A(i = feature, k = row)
            av = ok ? av : 0.0f;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                float bv = a.h3[rr * 256 + kb + 16 * t + n];                                             // B(k = row, j = input)
                bv = ok ? bv : 0.0f;
                ch[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, ch[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = acc[t] + ch[t];
        float bc = 0.0f;                                                                                 // db: the tile's rows in ascending order
#pragma unroll 4
        for (int j = 0; j < TR; ++j) {
            const bool ok = r0 + j < a.rows;
            const float v = a.g4[(size_t)(ok ? r0 + j : 0) * 16384 + f0 + n];
            bc = bc + (ok ? v : 0.0f);
        }
        bacc = bacc + bc;
    }
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float* d = a.grad + DH_W3 + (size_t)(f0 + 4 * q + e) * 256 + kb + 16 * t + n;               // D(i = 4 q + e, j = n)
            *d = a.first ? acc[t][e] : *d + acc[t][e];
        }
    if (kb == 0 && q == 0) {
        float* d = a.grad + DH_B3 + f0 + n;
        *d = a.first ? bacc : *d + bacc;
    }
}

// grid = 64 segments x 4: wave = 16 inputs k0 .. k0 + 15 of one segment of 256 features; part[seg][row][k] = sum_{f in seg} g4[row][f] W3[f][k]
__global__ void __launch_bounds__(256) k_dech_dh3(const DecHeadArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int seg = blockIdx.x >> 2;
    const int k0 = 16 * __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 3) * 4 + (int)(threadIdx.x >> 6));
    const int fs = seg * 256;
    const float* Wc = a.w + DH_W3 + (size_t)(fs + 4 * q) * 256 + k0 + n;
    float4 av[16];                                                                                      // A(i = input, k = feature): W3[fs + 16 c + 4 q + s][k0 + n]
#pragma unroll
    for (int c = 0; c < 16; ++c) av[c] = make_float4(Wc[(size_t)(16 * c) * 256], Wc[(size_t)(16 * c + 1) * 256], Wc[(size_t)(16 * c + 2) * 256], Wc[(size_t)(16 * c + 3) * 256]);
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        const int row = r0 + n;
        const bool ok = row < a.rows;
        const float* gp = a.g4 + (size_t)(ok ? row : 0) * 16384 + fs + 4 * q;
        const f32x4 sum = contract<8, 16>([&](int c) { return av[c]; }, [&](int c) {              // D(i = input 4 q + e, j = row n)
            float4 bv = *reinterpret_cast<const float4*>(gp + 16 * c);                                  // B(k = feature, j = row)
            if (!ok) bv = make_float4(0.f, 0.f, 0.f, 0.f);
            return bv;
        });
        if (ok) *reinterpret_cast<float4*>(a.part + ((size_t)seg * a.rows + row) * 256 + k0 + 4 * q) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
}

// grid = ceil(rows / 16): one 16-row tile; slab = the tile's index in its row group
// LDS: D = g_2 | H2 = x_2, then g_1 | H1 = x_1, then g_0 | X0 = s.
__global__ void __launch_bounds__(256) k_dech_small(const DecHeadArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float X0[TR * SLD];
    __shared__ __attribute__((aligned(16))) float D[TR * HLD];
    __shared__ __attribute__((aligned(16))) float H2[TR * HLD];
    __shared__ __attribute__((aligned(16))) float H1[TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, first = a.first;
    gfloat* slab = (gfloat*)a.slabs + (size_t)blockIdx.x * DEC_HEAD_SMALL_P;
    {
        const int r = tid >> 4, c = tid & 15;
        X0[r * SLD + c] = (r0 + r < a.rows && c < 10) ? a.s[(size_t)(r0 + r) * 10 + c] : 0.0f;
    }
#pragma unroll 1
    for (int r = 0; r < TR; ++r) {                       // thread = input k of row r: join of the 64 segment partials, gate of h3
        const int row = r0 + r, k = tid;
        float g = 0.0f, x2 = 0.0f, x1 = 0.0f;
        if (row < a.rows) {
            const float* pp = a.part + (size_t)row * 256 + k;
            const size_t ss = (size_t)a.rows * 256;
            float j8[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float sm = pp[(size_t)(8 * j) * ss];
#pragma unroll
                for (int i = 1; i < 8; ++i) sm = sm + pp[(size_t)(8 * j + i) * ss];
                j8[j] = sm;
            }
            const float sum = ((j8[0] + j8[1]) + (j8[2] + j8[3])) + ((j8[4] + j8[5]) + (j8[6] + j8[7]));
            g = gated(a.h3[(size_t)row * 256 + k], 2.0f * sum, true, true);
            x2 = a.h2[(size_t)row * 256 + k];
            x1 = a.h1[(size_t)row * 256 + k];
        }
        D[r * HLD + k] = g; H2[r * HLD + k] = x2; H1[r * HLD + k] = x1;
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 2; l >= 0; --l) {
        const int K = l == 0 ? 10 : 256;
        const gfloat* W = (const gfloat*)a.w + (l == 0 ? DH_W0 : l == 1 ? DH_W1 : DH_W2);
        gfloat* gW = slab + (l == 0 ? DH_W0 : l == 1 ? DH_W1 : DH_W2);
        gfloat* gB = slab + (l == 0 ? DH_B0 : l == 1 ? DH_B1 : DH_B2);
        const float* d = l == 2 ? D : l == 1 ? H2 : H1;            // g_l
        float* x = l == 2 ? H2 : l == 1 ? H1 : X0;                 // x_l
        const int xs = l == 0 ? SLD : HLD;
        dw_pass(d, HLD, x, xs, 256, K, gW, first, w, n, q);
        db_pass(d, HLD, 256, gB, first, tid);
        __syncthreads();                                           // dW_l has consumed x_l: it may now be overwritten
        if (l > 0) {
            dprev_pass<8, 16>(d, HLD, x, HLD, W, 256, 2.0f, true, w, n, q);
        } else if (w == 0 && a.ds) {                               // d_s[r][i] = sum_o g_0[r][o] W_0[o][i], no gate
            const float* dn = d + n * HLD + 4 * q;                 // B(k = o, j = row): g[n][16 c + 4 q + s]
            const f32x4 sum = contract<8, 16>([&](int c) {
                float av[4];                                       // A(i = input, k = o): W_0[16 c + 4 q + s][n]
#pragma unroll
                for (int s = 0; s < 4; ++s) av[s] = n < 10 ? W[(16 * c + 4 * q + s) * 10 + n] : 0.0f;
                return make_float4(av[0], av[1], av[2], av[3]);
            }, [&](int c) { return *reinterpret_cast<const float4*>(dn + 16 * c); });
            if (r0 + n < a.rows)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < 10) a.ds[(size_t)(r0 + n) * 10 + 4 * q + e] = sum[e];                // D(i = input 4 q + e, j = row n)
        }
        __syncthreads();
    }
}

// layers 0..2 do not depend on the geometry: train_dec_head_g.hip launches them on its own raw copy (a.w, a.s, a.h1 .. a.h3, a.rows, a.key)
void launch_dec_head_fwd_small(const DecHeadArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_dech_fwd, dim3((a.rows + TR - 1) / TR), dim3(256), 0, st, a);
}

void launch_dec_head_fwd(const DecHeadArgs& a, hipStream_t st) {
    launch_dec_head_fwd_small(a, st);
    hipLaunchKernelGGL(k_dech_fc4, dim3(16384 / 16 / 4), dim3(256), 0, st, a);
}

void launch_dec_head_gate(const float* h4, float* g, size_t n, hipStream_t st) {
    const int n4 = (int)(n / 4);
    hipLaunchKernelGGL(k_dech_gate, dim3((n4 + 255) / 256), dim3(256), 0, st, h4, g, n4);
}

void launch_dec_head_bwd(const DecHeadArgs& a, hipStream_t st) {
    launch_dec_head_gate(a.h4, a.g4, (size_t)a.rows * 16384, st);
    hipLaunchKernelGGL(k_dech_w4grad, dim3(16384 / 16 * 2 / 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dech_dh3, dim3(DEC_HEAD_SEGS * 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dech_small, dim3((a.rows + TR - 1) / TR), dim3(256), 0, st, a);
}

}  // namespace efe
