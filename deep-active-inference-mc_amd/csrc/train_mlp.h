// Device passes of the kernels that train a chain of Linear (+ ReLU, + MC-dropout) layers over 16-row tiles.  The k_dech_* kernels
// (train_dec_head.hip) are built of them; k_top_grad and k_mid_grad (train.hip) keep bodies of their own under the same order contract and
// share mfma4 only (why: at the kernels).  Every contraction is v_mfma_f32_16x16x4_f32 (exact fp32 fma chains),
// contraction off in the VALU code.  Lane (n, q) = (lane & 15, lane >> 4) of a wave feeds A(i = n, k = q) and B(k = q, j = n) and holds
// D(i = 4 q + e, j = n), e = 0..3.
//
// Order contract (what the fp64-rule tests, the frozen-bits test and tools/emulate_*.py rest on; a function of M alone):
//   chain    : a contraction over a layer's width runs on NACC accumulators.  16-channel chunk c goes to accumulator c & (NACC - 1) as four
//              MFMA steps (step s contracts channels 16 c + 4 q + s), chunks ascending; the accumulators are joined by tree<NACC>:
//              tree<2N>(a) = tree<N>(a[0..N)) + tree<N>(a[N..2N)).  NACC = 16 for the transition net, 8 for the decoder's head: different
//              bits at K = 256, never merged.  (k_top_grad keeps a chain of its own, stated there.)
//   tile     : a 16-row tile's contribution to a dW element is ONE 4-MFMA chain over its rows 0..15 ascending, to a db element the
//              sequential sum of its rows ascending.  Rows >= M hold exact zeros.
//   slab     : the one thread that owns an element writes (first) or adds the tile's contribution to its slab element, tiles ascending;
//              gradient = ((slab_0 + slab_1) + slab_2) + ... ascending (k_slab_sum / k_adam).  No float atomics.  Which tile goes to
//              which slab, and how many slabs there are, is stated at each kernel.
//   gate     : the backward gate keep * [a > 0] is READ OFF the stored activation, keep * [x > 0] (keep = 2 behind a dropout mask, else
//              1): no second Philox evaluation, and d_{l-1} overwrites x_l in place, lane (n, q) writing the four elements it reads.
#pragma once
#include "kernels.h"

namespace efe {
namespace mlp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
// a float in device memory: weights, biases and slabs reach the passes through pointers of this type, read from a layer table or formed
// in a register, which the compiler would otherwise address with flat loads and stores
typedef __attribute__((address_space(1))) float gfloat;

constexpr int TR = 16;                          // rows per tile

__device__ __forceinline__ void mfma4(f32x4& acc, float a0, float a1, float a2, float a3, const float4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b.w, acc, 0, 0, 0);
}

template <int N>
__device__ __forceinline__ f32x4 tree(const f32x4* a) {
#pragma clang fp contract(off)
    if constexpr (N == 1) return a[0];
    else return tree<N / 2>(a) + tree<N / 2>(a + N / 2);
}

// ---- dropout ---------------------------------------------------------------------------------------------------------
// the four mask words of Philox block `block` of (tag, row): feature f of a layer is bit f & 31 of word (f >> 5) & 3 of block f >> 7
__device__ __forceinline__ uint4 mask_block(const TrainKey& key, uint32_t tag, uint32_t block, uint32_t row) {
    // the key words pass through vector registers HERE: as loop invariants their ten Philox round keys are hoisted into twenty scalar
    // registers for the whole kernel, which then spills scalars
    uint32_t k0 = key.k0, k1 = key.k1;
    asm volatile("" : "+v"(k0), "+v"(k1));
    return noise_words(k0, k1, tag, block, key.row0 + row, key.stream, key.stage);
}
__device__ __forceinline__ uint32_t pick(const uint4& r, int w) { return w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w; }
__device__ __forceinline__ uint32_t mask_word(const uint4& r, int f0) { return pick(r, (f0 >> 5) & 3); }

// ReLU and mask of one pre-activation: the stored value is relu(v) * keep * 2
__device__ __forceinline__ float relu_drop(float v, bool relu, bool drop, uint32_t word, int bit) {
#pragma clang fp contract(off)
    if (relu) v = relu_nan(v);
    if (drop) v = v * keep2(((word >> bit) & 1u));
    return v;
}

// ---- the chain -------------------------------------------------------------------------------------------------------
// sum over the NC chunks c of A(c) B(c), unrolled: lda(c) -> the lane's A operands of the four steps of chunk c, ldb(c) -> its B operands
template <int NACC, int NC, class LA, class LB>
__device__ __forceinline__ f32x4 contract(LA lda, LB ldb) {
    f32x4 acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = (f32x4)(0.f);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float4 av = lda(c), bv = ldb(c);
        mfma4(acc[c & (NACC - 1)], av.x, av.y, av.z, av.w, bv);
    }
    return tree<NACC>(acc);
}

// bias, ReLU and mask of a forward tile: lane (n, q) holds features f0 + 4 q + e of row n -> the stored activation, zero beyond O
__device__ __forceinline__ float4 fwd_epilogue(const f32x4& sum, const gfloat* B, int f0, int q, int O, bool relu, bool drop, uint32_t word) {
#pragma clang fp contract(off)
    float4 out;
    float* o4 = &out.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int f = f0 + 4 * q + e;
        const float v = relu_drop(sum[e] + B[f < O ? f : 0], relu, drop, word, f & 31);
        o4[e] = f < O ? v : 0.0f;
    }
    return out;
}

// ---- backward passes over one tile in LDS: d [16][dld] = g_l, x [16][xld] = x_l (whole 16-column tiles, zero beyond the widths) ----
// dW[o][i] (+)= sum_r d[r][o] x[r][i]: wave w takes output tiles w, w + 4, ...; A(i = o, k = row) stays in registers over the i tiles
__device__ __forceinline__ void dw_pass(const float* d, int dld, const float* x, int xld, int O, int K, gfloat* gW, bool first, int w, int n, int q) {
#pragma clang fp contract(off)
    const int IT = (K + 15) / 16, OT = (O + 15) / 16;
#pragma unroll 1
    for (int ot = w; ot < OT; ot += 4) {
        const int o0 = 16 * ot;
        float av[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) av[c] = d[(4 * c + q) * dld + o0 + n];
#pragma unroll 2
        for (int it = 0; it < IT; ++it) {
            const int i0 = 16 * it;
            f32x4 acc = (f32x4)(0.f);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], x[(4 * c + q) * xld + i0 + n], acc, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = o0 + 4 * q + e, i = i0 + n;
                if (o < O && i < K) {
                    gfloat* p = gW + (size_t)o * K + i;
                    *p = first ? acc[e] : *p + acc[e];
                }
            }
        }
    }
}

// db[o] (+)= sum_r d[r][o], thread = o
__device__ __forceinline__ void db_pass(const float* d, int dld, int O, gfloat* gB, bool first, int tid) {
#pragma clang fp contract(off)
#pragma unroll 1
    for (int o = tid; o < O; o += 256) {
        float sm = d[o];
#pragma unroll
        for (int r = 1; r < TR; ++r) sm = sm + d[r * dld + o];
        gB[o] = first ? sm : gB[o] + sm;
    }
}

// d_prev[r][i] = (sum_o d[r][o] W[o][i]) * keep [x[r][i] > 0], written over x[r][i]; W [O][K] row-major, K a multiple of 16.  Each wave
// takes a contiguous quarter of the input tiles; O = 16 NC, or (BOUND) O < 16 NC rows of W: the features from O on feed exact zeros, never
// what lies behind W (d holds zeros there as well)
template <int NACC, int NC, bool BOUND = false>
__device__ __forceinline__ void dprev_pass(const float* d, int dld, float* x, int xld, const gfloat* W, int K, float keep, bool relu,
                                           int w, int n, int q, int O = 16 * NC) {
#pragma clang fp contract(off)
    const int IT = (K + 15) / 16, tpw = (IT + 3) / 4, t1 = min(IT, (w + 1) * tpw);
    const float* dn = d + n * dld + 4 * q;                             // B(k = o, j = row): d[n][16 c + 4 q + s]
#pragma unroll 1
    for (int t = w * tpw; t < t1; ++t) {
        const int i0 = 16 * t;
        const gfloat* Wc = W + i0 + n;                                 // A(i = input feature, k = o): W[16 c + 4 q + s][i0 + n]
        const f32x4 sum = contract<NACC, NC>(
            [&](int c) {
                const int o = 16 * c + 4 * q;
                float av[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if constexpr (BOUND) {
                        const bool in = o + s < O;
                        const float v = Wc[(size_t)(in ? o + s : 0) * K];
                        av[s] = in ? v : 0.0f;
                    } else av[s] = Wc[(size_t)(o + s) * K];
                }
                return make_float4(av[0], av[1], av[2], av[3]);
            },
            [&](int c) { return *reinterpret_cast<const float4*>(dn + 16 * c); });
        float* hp = x + n * xld + i0 + 4 * q;
        const float4 h = *reinterpret_cast<const float4*>(hp);
        float4 g;
        g.x = gated(h.x, keep * sum[0], relu, keep != 1.0f);
        g.y = gated(h.y, keep * sum[1], relu, keep != 1.0f);
        g.z = gated(h.z, keep * sum[2], relu, keep != 1.0f);
        g.w = gated(h.w, keep * sum[3], relu, keep != 1.0f);
        *reinterpret_cast<float4*>(hp) = g;
    }
}

}  // namespace mlp
}  // namespace efe
