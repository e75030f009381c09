// train_dec_head.hip at every admitted geometry: forward for training and backward of the decoder's dense head po_net[0:12]
// (the reference's torchmodel.py:107-118) with the width of po_net.9 taken from the context, F = 64 B^2 (B = the decoder's base grid,
// 9 .. 32: F = 5 184 .. 65 536).  With train_dec_g.hip's tail: the gradient of the reconstruction term with respect to every decoder
// parameter and to s at C x R x R.  The mathematics, the chains (contract<8, 16>, tree<8>) and train_mlp.h's tile, slab and gate rules are
// train_dec_head.hip's; only what depends on F is restated here.  W_l comes from the raw copy in parameters() order (DecHeadGeo), h4 is
// stored in the reference's order f = c B^2 + p, which launch_dec_tail_g_group consumes.
//
// Layers 0..2 (10-256-256-256) do not depend on the geometry: k_dech_fwd runs them as it is (launch_dec_head_fwd_small), and k_dech_gate
// gates d_h4.  New kernels, one row group of at most DecTailGeo::rows_per_pass() rows (64 while B <= 16, else 32) per launch:
//   k_dechg_fc4   : layer 3; one wave = 16 consecutive reference features (its 16 x 256 weights stay in registers) x every 16-row tile.
//   k_dechg_w4grad: dW_3, db_3; one wave owns 16 features x 128 inputs (K = the rows), written / added into the caller's gradient.
//   k_dechg_dh3   : partial sums of g_3 W_3 over S = ceil(F / 256) segments of 256 features; one wave = 16 inputs of one segment.
//   k_dechg_join  : joins the S partials of a (row, input) and gates by 2 [h3 > 0]: g_2, one workgroup per row (a kernel of its own: the S
//                   dependent loads per element are latency, spread here over `rows` workgroups, not over the four of k_dechg_small).
//   k_dechg_small : runs layers 2, 1, 0 backward from g_2 over one 16-row tile in LDS.
//
// Layer 3's mask: the forward decoder (k_fc4_g) keys the bit of reference feature f = c B^2 + p by the NHWC feature f' = p 64 + c: block
// f' >> 7 = p >> 1, word 2 (p & 1) + (c >> 5), bit c & 31.  B^2 need not be a multiple of 16 (81, 100, 441): a wave's 16 features may
// straddle a channel boundary, c stepping and p wrapping to 0 inside the tile, so (c, p) is formed PER FEATURE and every feature draws its
// own block.  The value of a feature is one contract<8, 16> over K = 256 whatever the tiling.
//
// Reduction order, a function of the geometry and M alone (every element has ONE owning thread, no float atomics):
//   rows     : row group g = rows P g .. P g + P - 1, P = rows_per_pass(); 16-row tile t = rows 16 t .. 16 t + 15 of the CALL (P is a
//              multiple of 16); rows >= M contribute exact zeros: a padding lane's address is clamped to the group's row 0 and both its MFMA
//              operands are zero.
//   dW_3/db_3: per element and group, the tiles ascending: chunk = one 16-term MFMA chain over the tile's rows (db: a sequential sum),
//              group = ((chunk_0 + chunk_1) + chunk_2) + chunk_3, or chunk_0 + chunk_1 in a 32-row group; gradient = ((group_0 + group_1)
//              + ...) ascending, in place.
//   d_h3     : per row: segment j = features 256 j .. 256 j + 255 = tree<8> of eight 32-term chains; for odd B the last segment holds 64
//              features, its chunks 4 .. 15 feeding exact zeros into both operands (address clamped to the segment's chunk 0).  The S
//              segments are joined as sequential sums of runs of eight consecutive segments, ascending, the last run shorter; the runs
//              are then added in ascending order, ((run_0 + run_1) + run_2) + ...  (Not train_dec_head.hip's tree<8> of eight runs: equal
//              bits with efe_dec_grad at 1 x 64 x 64 are not promised.)
//   layers 0..2: G = min(ceil(M / 16), DEC_HEAD_SLABS = 4) slabs of 134 400 floats; tile t of the call adds its 16-term chain (db:
//              sequential sum) to slab t mod 4, tiles ascending (the first four tiles write); gradient = ((slab_0 + slab_1) + slab_2) + slab_3.
// Two identical calls give identical bits; h1..h4, d_s (and through the tail po1, nlogpo1) of a row depend on that row and its global row
// id only.
#include "train_mlp.h"

namespace efe {

using namespace mlp;

namespace {

constexpr int HLD = 256 + 4;       // LDS row stride of a 256-wide activation
constexpr int SLD = 16 + 4;        // ... of the input tile s (10 columns, zero up to 16)

}  // namespace

// grid = B^2 workgroups: wave = 16 consecutive reference features f0 .. f0 + 15 (F / 16 = 4 B^2 waves)
__global__ void __launch_bounds__(256) k_dechg_fc4(const DecHeadGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int f0 = 16 * __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int F = a.geo.F(), BB = a.geo.BB();
    const float4* Wp = reinterpret_cast<const float4*>(a.w + DH_W3 + (size_t)(f0 + n) * 256 + 4 * q);
    float4 av[16];                                                                                      // A(i = feature, k): W[f0 + n][16 c + 4 q + s]
#pragma unroll
    for (int c = 0; c < 16; ++c) av[c] = Wp[4 * c];
    const float4 bias = *reinterpret_cast<const float4*>(a.w + a.geo.b3() + f0 + 4 * q);
    // this lane's features f0 + 4 q + e = c B^2 + p: block p >> 1, word 2 (p & 1) + (c >> 5), bit c & 31, each feature on its own
    uint32_t blk[4];
    int wrd[4], bit[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int f = f0 + 4 * q + e, ch = f / BB, p = f - ch * BB;
        blk[e] = (uint32_t)(p >> 1); wrd[e] = 2 * (p & 1) + (ch >> 5); bit[e] = ch & 31;
    }
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
        const float b4[4] = {bias.x, bias.y, bias.z, bias.w};
        float4 out;
        float* o4 = &out.x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t keep = pick(mask_block(a.key, TAG_DEC + 3u, blk[e], (uint32_t)row), wrd[e]);
            o4[e] = relu_drop(sum[e] + b4[e], true, true, keep, bit[e]);
        }
        if (ok) *reinterpret_cast<float4*>(a.h4 + (size_t)row * F + f0 + 4 * q) = out;                  // D(i = 4 q + e, j = n)
    }
}

// grid = 2 B^2 workgroups: wave = 16 features x 128 inputs of dW_3 (and, in the first half, the 16 features of db_3)
__global__ void __launch_bounds__(256) k_dechg_w4grad(const DecHeadGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int f0 = 16 * (wv >> 1), kb = 128 * (wv & 1);
    const size_t F = (size_t)a.geo.F();
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
            float av = a.g4[rr * F + f0 + n];                                                            // A(i = feature, k = row)
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
            const float v = a.g4[(size_t)(ok ? r0 + j : 0) * F + f0 + n];
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
        float* d = a.grad + a.geo.b3() + f0 + n;
        *d = a.first ? bacc : *d + bacc;
    }
}

// grid = S segments x 4: wave = 16 inputs k0 .. k0 + 15 of one segment of 256 features; part[seg][row][k] = sum_{f in seg} g4[row][f] W3[f][k].
// A chunk of 16 features lies wholly inside F or wholly behind it (F is a multiple of 64)
__global__ void __launch_bounds__(256) k_dechg_dh3(const DecHeadGArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int seg = blockIdx.x >> 2;
    const int k0 = 16 * __builtin_amdgcn_readfirstlane((int)(blockIdx.x & 3) * 4 + (int)(threadIdx.x >> 6));
    const int F = a.geo.F(), fs = seg * 256;
    const int nc = min(16, (F - fs) >> 4);                                                              // chunks of this segment inside F: 16, or 4
    const float* Wc = a.w + DH_W3 + (size_t)(fs + 4 * q) * 256 + k0 + n;
    float4 av[16];                                                                                      // A(i = input, k = feature): W3[fs + 16 c + 4 q + s][k0 + n]
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const bool in = c < nc;
        const size_t o = (size_t)(in ? 16 * c : 0) * 256;
        const float4 v = make_float4(Wc[o], Wc[o + 256], Wc[o + 512], Wc[o + 768]);
        av[c] = in ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll 1
    for (int r0 = 0; r0 < a.rows; r0 += TR) {
        const int row = r0 + n;
        const bool ok = row < a.rows;
        const float* gp = a.g4 + (size_t)(ok ? row : 0) * F + fs + 4 * q;
        const f32x4 sum = contract<8, 16>([&](int c) { return av[c]; }, [&](int c) {              // D(i = input 4 q + e, j = row n)
            const bool in = ok && c < nc;
            float4 bv = *reinterpret_cast<const float4*>(gp + (c < nc ? 16 * c : 0));                   // B(k = feature, j = row)
            if (!in) bv = make_float4(0.f, 0.f, 0.f, 0.f);
            return bv;
        });
        if (ok) *reinterpret_cast<float4*>(a.part + ((size_t)seg * a.rows + row) * 256 + k0 + 4 * q) = make_float4(sum[0], sum[1], sum[2], sum[3]);
    }
}

// grid = rows: thread = input k of one row.  g_2[row][k] = (join of the S segment partials) * 2 [h3 > 0], left in plane 0 of `part`: the
// element's one owner reads its S partials, then overwrites the first.  Eight loads of a run are in flight at once; a segment >= S of the last
// run reads the run's first segment and is not added
__global__ void __launch_bounds__(256) k_dechg_join(const DecHeadGArgs a) {
#pragma clang fp contract(off)
    const int row = blockIdx.x, k = threadIdx.x, S = a.geo.segs();
    float* pp = a.part + (size_t)row * 256 + k;
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
    *pp = gated(a.h3[(size_t)row * 256 + k], 2.0f * sum, true, true);
}

// grid = ceil(rows / 16): one 16-row tile; slab = the tile's index in the CALL mod DEC_HEAD_SLABS (a.tile0 + blockIdx.x: the tiles of one
// launch go to different slabs), written by the call's first four tiles, added to by the later ones
// LDS: D = g_2 | H2 = x_2, then g_1 | H1 = x_1, then g_0 | X0 = s.
__global__ void __launch_bounds__(256) k_dechg_small(const DecHeadGArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float X0[TR * SLD];
    __shared__ __attribute__((aligned(16))) float D[TR * HLD];
    __shared__ __attribute__((aligned(16))) float H2[TR * HLD];
    __shared__ __attribute__((aligned(16))) float H1[TR * HLD];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = blockIdx.x * TR, gt = a.tile0 + (int)blockIdx.x, first = gt < DEC_HEAD_SLABS;
    gfloat* slab = (gfloat*)a.slabs + (size_t)(gt % DEC_HEAD_SLABS) * DEC_HEAD_SMALL_P;
    {
        const int r = tid >> 4, c = tid & 15;
        X0[r * SLD + c] = (r0 + r < a.rows && c < 10) ? a.s[(size_t)(r0 + r) * 10 + c] : 0.0f;
    }
#pragma unroll 1
    for (int r = 0; r < TR; ++r) {                       // thread = input k of row r: g_2 as k_dechg_join left it
        const int row = r0 + r, k = tid;
        float g = 0.0f, x2 = 0.0f, x1 = 0.0f;
        if (row < a.rows) {
            g = a.part[(size_t)row * 256 + k];
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

void launch_dec_head_g_fwd(const DecHeadGArgs& a, hipStream_t st) {
    DecHeadArgs h{};
    h.w = a.w; h.s = a.s; h.h1 = a.h1; h.h2 = a.h2; h.h3 = a.h3; h.rows = a.rows; h.key = a.key;
    launch_dec_head_fwd_small(h, st);
    hipLaunchKernelGGL(k_dechg_fc4, dim3(a.geo.BB()), dim3(256), 0, st, a);
}

void launch_dec_head_g_bwd(const DecHeadGArgs& a, hipStream_t st) {
    launch_dec_head_gate(a.h4, a.g4, (size_t)a.rows * a.geo.F(), st);
    hipLaunchKernelGGL(k_dechg_w4grad, dim3(2 * a.geo.BB()), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dechg_dh3, dim3(a.geo.segs() * 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dechg_join, dim3(a.rows), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_dechg_small, dim3((a.rows + TR - 1) / TR), dim3(256), 0, st, a);
}

}  // namespace efe
