// Fused decoder kernels for gfx950: the three ConvTranspose2d + ReLU layers, the final
// ConvTranspose2d(32,1) + Sigmoid and the per-image EFE reductions of
// /root/reference/src/torchmodel.py:120-127 (po_net.13..20), torchutils.py:26-37, torchmodel.py:210-212,289,292.
//
// One workgroup (4 waves) owns one decoder image; activations live in LDS between layers:
//
//   k_dec_a :  x4[16x16x64] --LDS--> ConvT(64,64,s1)+ReLU (Winograd F(2x2,3x3)) --LDS (in place)--> ConvT(64,64,s2)+ReLU (F(2,2), registers) --> y2[32x32x64] (HBM)
//   k_dec_b4:  y2 strips --LDS--> ConvT(64,32,s2)+ReLU (F(2,2), registers) --MFMA--> tap values of the 32->1 conv, horizontal sums in registers
//              --LDS ring of H planes--> vertical gather + sigmoid + entropy / reward reduction (+ optional image store)
//   k_dec_a_s / k_dec_b4<4>: the same kernels with an image over eight / four workgroups, for launches of <= 128 images
//
// LDS images are [pixel][17 float4 slots]: the 16 channel quads of a pixel plus one slot of padding, so that the ds_read_b128 of an
// MFMA B fragment (32 pixels x same quad) is bank-conflict free (16 consecutive pixels cover the 16 bank quads: 17 p mod 16 = p) and a
// fragment address is pixel base + an immediate (k_fc4's batch tile alone is still XOR-swizzled).  Weights are read as pre-packed A
// fragments straight from L2 (1 KiB coalesced per wave-load, shared by all workgroups).  fp32 MFMA (v_mfma_f32_32x32x2_f32 for ConvT1 and
// k_fc4, v_mfma_f32_16x16x4_f32 for the two F(2, 2) layers and the 32 -> 1 conv): exact fp32 numerics.
#include <utility>
#include "mfma_pipe.h"

namespace efe {

// ---------------------------------------------------------------------------------------------------------
// The stride-2 layers ConvT2 (ConvTranspose2d(64, 64, 3, s2, p1, op1): f22_l2 in k_dec_a / k_dec_a_s) and ConvT3 (ConvTranspose2d(64, 32, 3, s2,
// p1, op1): k_dec_b4) by per-parity minimal filtering F(2, 2).  Along one dimension, with taps g0, g1, g2 (oh = 2 ih - 1 + kh) and x = 0
// behind the last row / column, output 2m = x[m] g1 and 2m + 1 = x[m] g2 + x[m + 1] g0.  For an input pair block u
// (x0 = x[2u], x1 = x[2u + 1], x2 = x[2u + 2]) the views d0 = x0 - x1, d1 = x1, d2 = x2 - x1 give the four outputs 4u .. 4u + 3 from
// five products instead of six:
//     P1 = d0 g1 -> 0    P2 = d1 g1 -> 0, 2    P3 = d0 g2 -> 1    P4 = d1 (g0 + g2) -> 1, 3    P5 = d2 g0 -> 3
// In 2D (the outer product of this table with itself) a 2 x 2 input block needs 25 products instead of 36: 9 views d_a (x) d_b and 16
// weight matrices U = w_r (x) w_c, w in {g1, g2, g0 + g2, g0}, formed in fp64 at commit time and rounded once (engine_weights.hip).  The 9
// products with one output in both dimensions chain straight into that output; the other 16 run in a short-lived accumulator that is
// then added into its 2 or 4 outputs.  (The 1D table f22_* is in kernels.h: engine_weights.hip forms the weights from it.)
//
// compile-time loop: f(std::integral_constant<int, 0>{}) .. f(std::integral_constant<int, N - 1>{})
template <class F, int... I> __device__ __forceinline__ void static_for_(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for_(f, std::make_integer_sequence<int, N>{}); }

// The schedule of both layers: six groups of products that share their views (every B fragment read feeds 4 or 5 independent chains):
//   G0 V(0,0): (P1|P3) x (P1|P3)  direct      G1 V(0,1): (P1|P3) x (P2|P4)      G2 V(1,0): (P2|P4) x (P1|P3)      G3 V(1,1): (P2|P4) x (P2|P4)
//   G4 V(1,2), V(2,1), V(2,2): (P2|P4) x P5, P5 x (P2|P4), P5 x P5 (direct)      G5 V(0,2), V(2,0): (P1|P3) x P5, P5 x (P1|P3)  direct
// w3_prod(G, c) = 5 pr + pc of chain c of group G (rows x columns)
__host__ __device__ constexpr int w3_nch(int G) { return G == 4 ? 5 : 4; }
__host__ __device__ constexpr int w3_prod(int G, int c) {
    return G < 4 ? 5 * ((G >> 1) + 2 * (c >> 1)) + (G & 1) + 2 * (c & 1)
         : G == 4 ? (c < 2 ? 5 * (1 + 2 * c) + 4 : c < 4 ? 20 + 1 + 2 * (c - 2) : 24)
                  : (c < 2 ? 5 * (2 * c) + 4 : 20 + 2 * (c - 2));
}
__host__ __device__ constexpr bool w3_direct(int pp) { return f22_o1(pp / 5) < 0 && f22_o1(pp % 5) < 0; }
__host__ __device__ constexpr int w3_view(int pp) { return 3 * f22_view(pp / 5) + f22_view(pp % 5); }
__host__ __device__ constexpr int w3_mat(int pp) { return 4 * f22_wt(pp / 5) + f22_wt(pp % 5); }
__host__ __device__ constexpr bool w3_hits(int pp, int o) {          // product pp feeds output o = 4 orow + ocol of the block
    const int r = o >> 2, c = o & 3, pr = pp / 5, pc = pp % 5;
    return (r == f22_o0(pr) || r == f22_o1(pr)) && (c == f22_o0(pc) || c == f22_o1(pc));
}
// output o already holds a value when chain c of group G reaches it (a group's direct chains run before its temporaries are added,
// those in chain order): otherwise the chain starts from the bias (direct: the C operand of its first MFMA; temporary: bias + M)
__host__ __device__ constexpr bool w3_seen(int G, int c, int o) {
    for (int g = 0; g < G; ++g)
        for (int k = 0; k < w3_nch(g); ++k) if (w3_hits(w3_prod(g, k), o)) return true;
    if (!w3_direct(w3_prod(G, c)))
        for (int k = 0; k < w3_nch(G); ++k)
            if ((w3_direct(w3_prod(G, k)) || k < c) && w3_hits(w3_prod(G, k), o)) return true;
    return false;
}
__host__ __device__ constexpr bool w3_uses_view(int G, int vi) {
    for (int k = 0; k < w3_nch(G); ++k) if (w3_view(w3_prod(G, k)) == vi) return true;
    return false;
}
__host__ __device__ constexpr bool f22_in(int a, int r) { return a == 0 ? r <= 1 : (a == 1 ? r == 1 : r >= 1); }   // view a reads x_r
__host__ __device__ constexpr bool w3_reads(int G, int r, int c) {   // input pixel (r, c) of the 3 x 3 block neighbourhood
    for (int vi = 0; vi < 9; ++vi) if (w3_uses_view(G, vi) && f22_in(vi / 3, r) && f22_in(vi % 3, c)) return true;
    return false;
}

// The contraction of one tile, shared by both layers: 24 steps ST = (group ST >> 2, channel chunk ST & 3), every index a compile-time
// constant, software-pipelined: a step forms its group's views from the raw neighbourhood xr, takes its A fragments out of the ring aq
// (PD steps deep; filled for steps 0 .. PD - 1 on entry) and requests the fragments of step ST + PD and the pixels of step ST + 1 in
// front of its own MFMAs (e outer, chain inner: every B value feeds 4 or 5 independent chains).
//   wf(m, kc, next): the A fragment of matrix m, chunk kc; next: the step requested lies behind this tile (ST + PD >= 24).  WRAP: those
//   steps are requested too (the next tile's first fragments: aq holds them on exit); otherwise the ring runs dry.
//   px(i, jj, kc): pixel (i, jj) of the lane's 3 x 3 neighbourhood, the lane's quad of chunk kc.
//   piece(stc): the caller's own non-matrix work of step stc, behind prio_nonmatrix().
//   OPAQUE: views and temporaries go through sub4 / add4 (mfma_pipe.h: single-lane instructions) instead of the vector operators.
//   LATE: a group's temporaries are added a step later, behind the next step's views and requests and in front of its MFMAs (the first
//   that may touch those outputs again; the last group's behind the loop), not right behind the group's last MFMA: there every add waits
//   out that MFMA's result latency in hazard wait states.  The order per output element is the same either way.
template <int PD, bool LATE, bool OPAQUE, bool WRAP, class WF, class PX, class Piece>
__device__ __forceinline__ void f22_contract(f32x4 (&acc)[16], f32x4 (&aq)[PD][5], const f32x4 bias4, WF wf, PX px, Piece piece) {
    constexpr int NST = 24;                            // contraction steps: 6 groups x 4 chunks of 16 channels
    auto sub = [](const f32x4 a, const f32x4 b) -> f32x4 { if constexpr (OPAQUE) return sub4(a, b); else return a - b; };
    auto add = [](const f32x4 a, const f32x4 b) -> f32x4 { if constexpr (OPAQUE) return add4(a, b); else return a + b; };
    // view (a, b) of the raw neighbourhood x[i][jj]: the columns first (x[i][0] - x[i][1] | x[i][1] | x[i][2] - x[i][1]), then the rows
    // in the same form
    auto view = [&](const f32x4 (&x)[9], int vi) -> f32x4 {
        const int va = vi / 3, vb = vi % 3;
        auto cv = [&](int i) -> f32x4 { return vb == 0 ? sub(x[3 * i], x[3 * i + 1]) : (vb == 1 ? x[3 * i + 1] : sub(x[3 * i + 2], x[3 * i + 1])); };
        return va == 0 ? sub(cv(0), cv(1)) : (va == 1 ? cv(1) : sub(cv(2), cv(1)));
    };
    const f32x4 zero4 = {};
    f32x4 tq[5], xr[9];
    static_for<9>([&](auto i) { if constexpr (w3_reads(0, i / 3, i % 3)) xr[i] = px(i / 3, i % 3, 0); });
    // group GG's temporaries into their outputs, in chain order
    auto add_tmp = [&](auto gg) {
        constexpr int GG = decltype(gg)::value;
        static_for<w3_nch(GG)>([&](auto c) {
            constexpr int PP = w3_prod(GG, c);
            if constexpr (!w3_direct(PP))
                static_for<16>([&](auto o) {
                    if constexpr (w3_hits(PP, o)) {
                        if constexpr (w3_seen(GG, c, o)) acc[o] = add(acc[o], tq[c]);
                        else acc[o] = add(bias4, tq[c]);
                    }
                });
        });
    };
    static_for<NST>([&](auto stc) {
        constexpr int ST = decltype(stc)::value, G = ST >> 2, KC = ST & 3, GN = (ST + 1) >> 2, KN = (ST + 1) & 3;
        constexpr int SP = (ST + PD) % NST, GP = SP >> 2, KP = SP & 3;      // the step whose fragments are requested now
        f32x4 vw[9], ac[5];
        static_for<9>([&](auto vi) { if constexpr (w3_uses_view(G, vi)) vw[vi] = view(xr, vi); });
#pragma unroll
        for (int c = 0; c < 5; ++c) ac[c] = aq[ST % PD][c];
        if constexpr (WRAP || ST + PD < NST)
            static_for<w3_nch(GP)>([&](auto c) { aq[ST % PD][c] = wf(w3_mat(w3_prod(GP, c)), KP, ST + PD >= NST); });
        if constexpr (ST + 1 < NST)
            static_for<9>([&](auto i) { if constexpr (w3_reads(GN, i / 3, i % 3)) xr[i] = px(i / 3, i % 3, KN); });
        if constexpr (LATE && KC == 0 && ST > 0) {     // (the barrier keeps hipcc from moving the adds back up)
            __builtin_amdgcn_sched_barrier(0);
            add_tmp(std::integral_constant<int, (ST > 0 ? G - 1 : 0)>{});
        }
        prio_matrix();
        __builtin_amdgcn_sched_barrier(0);             // keep the prefetch loads AHEAD of this step's MFMAs
#pragma unroll
        for (int e = 0; e < 4; ++e)
            static_for<w3_nch(G)>([&](auto c) {
                constexpr int PP = w3_prod(G, c);
                const float b = vw[w3_view(PP)][e], av = ac[c][e];
                if constexpr (w3_direct(PP)) {
                    constexpr int O = 4 * f22_o0(PP / 5) + f22_o0(PP % 5);
                    constexpr bool FIRST = KC == 0 && !w3_seen(G, c, O);
                    acc[O] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, (FIRST && e == 0) ? bias4 : acc[O], 0, 0, 0);
                } else {
                    tq[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, (KC == 0 && e == 0) ? zero4 : tq[c], 0, 0, 0);
                }
            });
        prio_nonmatrix();
        if constexpr (!LATE && KC == 3) add_tmp(std::integral_constant<int, G>{});
        piece(stc);
    });
    if constexpr (LATE) add_tmp(std::integral_constant<int, 5>{});      // (empty today: group 5 has direct chains only)
}

// ---------------------------------------------------------------------------------------------------------
// k_dec_a: ConvTranspose2d(64,64,3,s1,p1)+ReLU then ConvTranspose2d(64,64,3,s2,p1,op1)+ReLU, one image per WG.
// ---------------------------------------------------------------------------------------------------------
// The staged image takes DA_PS = 17 float4 slots per pixel (16 channel quads + 1 pad): 16 consecutive pixels cover the 16 bank quads
// (17 p mod 16 = p), and a fragment address is pixel base + constant -- the chunk offset is an immediate of the ds_read (the XOR swizzle
// of rounds 1-2 cost an XOR and an add per chunk and 11 % of the LDS cycles in bank conflicts).
constexpr int DA_PS = 17;
constexpr int DA_BIAS = 273 * DA_PS;       // float4 index of the two bias vectors behind the image + a zero row (pixels 256 .. 272: row 16, which layer 2's last block row reads as its x_2)

// ---------------------------------------------------------------------------------------------------------
// Layer 1 (ConvTranspose2d(64,64,3,s1,p1) = a 3x3 correlation with the flipped kernel g, pad 1) by Winograd F(2x2, 3x3) (Lavin):
//   output tile (ty, tx) = pixels (2ty + r, 2tx + c), r, c in {0, 1}; input tile d[i][jj] = x[2ty - 1 + i][2tx - 1 + jj] (zero outside)
//   xi = (a, b) in 4 x 4:  V_xi = (B^T d B)[a][b],  M_xi[co][tile] = sum_ci U_xi[co][ci] V_xi[ci][tile],  out[r][c] = bias + sum_xi AT[r][a] AT[c][b] M_xi
// U = G g G^T is formed in fp64 at commit time and rounded once (engine_weights.hip), packed like a 16-tap conv: [xi][2 tiles][8 chunks][64 lanes][4].
// Each row of B^T has two non-zero entries, the first +1: row a of B^T d is d[wino_i0(a)] + wino_s1(a) d[wino_i1(a)], so a B fragment is four LDS reads
// and three fp32 adds per component (a signed add is written as fma(+-1, x, y): exactly y +- x).  16 xi-GEMMs of 32 MFMAs per 32-channel x
// 32-tile block replace the 9 x 32 of the direct form.  The output transform runs in ascending xi = 4a + b, one signed add per non-zero AT
// coefficient (AT[r][a] AT[c][b] in {0, +-1}): out[r][c] sees the same operations, in the same order, whichever output rows a wave owns.
// NR = output rows R0 .. R0 + NR - 1 of the tiles this wave owns (2: k_dec_a; 1: k_dec_a_s, whose waves split the rows):
// only the xi rows a with AT[r][a] != 0 for one of them are contracted (r = 0: a = 0..2; r = 1: a = 1..3).
// pix(i, jj) -> LDS float4 index of input pixel (i, jj) of the lane's tile (the zero pixel outside the image).
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int wino_i0(int a) { return a == 0 ? 0 : (a == 2 ? 2 : 1); }     // B^T row a: +1 at wino_i0(a), wino_s1(a) at wino_i1(a)
__host__ __device__ constexpr int wino_i1(int a) { return a == 0 ? 2 : (a == 1 ? 2 : (a == 2 ? 1 : 3)); }
__host__ __device__ constexpr float wino_s1(int a) { return a == 1 ? 1.0f : -1.0f; }
__host__ __device__ constexpr float wino_at(int r, int a) { return r == 0 ? (a < 3 ? 1.0f : 0.0f) : (a == 0 ? 0.0f : (a == 1 ? 1.0f : -1.0f)); }   // AT = [[1,1,1,0],[0,1,-1,-1]]

__device__ __forceinline__ float4 fma4(float s, const float4& x, const float4& y) {          // y + s x per component (s = +-1: exactly y +- x)
    return make_float4(__builtin_fmaf(s, x.x, y.x), __builtin_fmaf(s, x.y, y.y), __builtin_fmaf(s, x.z, y.z), __builtin_fmaf(s, x.w, y.w));
}
// the transform of xi (a, b), whose GEMM is m, into the outputs
// (MASK: the output rows whose AT[r][a] is non-zero for this a -- a constant, so that no update is conditional at run time:
// hipcc turns a run-time skip into selects that hold every output twice)
template <int NR, int R0, int MASK>
__device__ __forceinline__ void wino_otrans(f32x16 (&out)[NR][2], const int a, const int b, const f32x16& m) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (!((MASK >> r) & 1)) continue;
        const float car = wino_at(R0 + r, a);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float cbc = wino_at(c, b);
            if (cbc == 0.0f) continue;
            const float cf = car * cbc;
#pragma unroll
            for (int e = 0; e < 16; ++e) out[r][c][e] = __builtin_fmaf(cf, m[e], out[r][c][e]);
        }
    }
}
template <int NR, int R0, class Pix>
__device__ __forceinline__ void wino_l1(f32x16 (&out)[NR][2], const float4* __restrict__ U, const float4* sm, const int h,
                                        const int mt_, Pix pix) {
    constexpr int PD = 4;                                   // A-fragment prefetch distance in chunks (4 MFMAs each; fragments come from L2)
    const unsigned ln = (threadIdx.x & 63u) * 16u;
    const __amdgpu_buffer_rsrc_t ur = wrsrc(U);
    // laundered per call: stops hipcc hoisting the ~80 constant fragment offsets of the peeled xi rows out of the image loop (SGPR spills)
    int mt = mt_; asm volatile("" : "+s"(mt));
    constexpr int a_lo = NR == 2 ? 0 : R0, a_hi = NR == 2 ? 4 : R0 + 3;
    // A fragment of chunk kc of xi (a, b): byte offset a * 64 KiB + (2 b + mt) * 8 KiB + kc * 1 KiB (one scalar base per a + a literal)
    auto ufrag = [&](int a, int b, int kc) { return wfrag(ur, ln, (size_t)(((4 * a + b) * 2 + mt) * 8 + kc) * 64); };
    auto bases = [&](int a, int b, int (&pb)[4]) {          // d[i0][j0], d[i0][j1], d[i1][j0], d[i1][j1] of xi (a, b)
        const int i0 = wino_i0(a), i1 = wino_i1(a), j0 = wino_i0(b), j1 = wino_i1(b);
        pb[0] = pix(i0, j0); pb[1] = pix(i0, j1); pb[2] = pix(i1, j0); pb[3] = pix(i1, j1);
    };
    float4 aq[PD], raw[4];
    int pb[4];
#pragma unroll
    for (int p = 0; p < PD; ++p) aq[p] = ufrag(a_lo, 0, p);
    bases(a_lo, 0, pb);
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = sm[pb[q] + h];
    f32x16 xacc;
    const f32x16 zero = {};
    auto xi_row = [&](int a, auto mask) {               // the four xi (a, 0..3)
        const float s1 = wino_s1(a);
        const int an = a + 1 < a_hi ? a + 1 : a;        // the next xi row (the last one re-reads its own fragments: never used)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float t1 = wino_s1(b);
#pragma unroll
            for (int kc = 0; kc < 8; ++kc) {
                const float4 av = aq[kc % PD];
                aq[kc % PD] = (b * 8 + kc + PD < 32) ? ufrag(a, (b * 8 + kc + PD) >> 3, (kc + PD) & 7) : ufrag(an, 0, (kc + PD) & 7);
                // V fragment of this chunk: (d00 + s1 d10) + t1 (d01 + s1 d11), per component (c0, then c1: nested calls are evaluated in another order)
                const float4 c0 = fma4(s1, raw[2], raw[0]), c1 = fma4(s1, raw[3], raw[1]);
                const float4 v = fma4(t1, c1, c0);
                // the next chunk's input pixels (the next xi's first chunk behind the last one)
                if (kc < 7) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) raw[q] = sm[pb[q] + 2 * (kc + 1) + h];
                } else {
                    if (b < 3) bases(a, b + 1, pb);
                    else bases(an, 0, pb);
#pragma unroll
                    for (int q = 0; q < 4; ++q) raw[q] = sm[pb[q] + h];
                }
                prio_matrix();
                __builtin_amdgcn_sched_barrier(0);      // keep the prefetch loads AHEAD of this chunk's MFMAs
                f32x16& x = xacc;
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, v.x, kc == 0 ? zero : x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, v.y, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, v.z, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, v.w, x, 0, 0, 0);
                prio_nonmatrix();
            }
            // the xi's output transform, behind its last MFMA.  (A second accumulator, with this transform spread over the next xi's
            // chunks, fits all three kernels -- 244 / 219 / 252 VGPRs, unchanged -- and was measured in k_dec_ab: the same cycles
            // within the parent's own spread, profiles/r14_overlap_items.txt.  The drain is 16 x 64 cycles per image and the partner
            // wave fills most of it; what layer 1 pays for is the number of non-matrix instructions: see wino_l1_rows.)
            wino_otrans<NR, R0, decltype(mask)::value>(out, a, b, xacc);
        }
    };
    if constexpr (NR == 2) {                            // a = 0: row 0 only; a = 1, 2: both; a = 3: row 1 only
        xi_row(0, std::integral_constant<int, 1>{});
#pragma unroll 1
        for (int a = 1; a < 3; ++a) xi_row(a, std::integral_constant<int, 3>{});
        xi_row(3, std::integral_constant<int, 2>{});
    } else {
#pragma unroll 1
        for (int a = a_lo; a < a_hi; ++a) xi_row(a, std::integral_constant<int, 1>{});
    }
}
// k_dec_ab's form of layer 1 (NR = 2, R0 = 0): the four xi (a, 0..3) of a row are contracted TOGETHER, chunk by chunk, into four
// accumulators.  They share their row transform: per chunk the two input rows wino_i0(a), wino_i1(a) are read once for the tile's four
// columns (8 LDS reads where four xi on their own take 16) and col[j] = d[i0][j] + s1 d[i1][j] is formed once (16 + 4 x 4 fmas where
// they take 4 x 12); xi (a, b)'s fragment is col[j0] + t1 col[j1], which is (d00 + s1 d10) + t1 (d01 + s1 d11) as in wino_l1, operation
// for operation.  Every xi-GEMM still runs over chunks 0..7 on its own accumulator and the output transforms follow in ascending xi at
// the row's end, so an output element sees what it sees in wino_l1: the same bits.  The 48 more accumulator registers and 16 more of
// raw pixels are there in k_dec_ab alone, whose next image is not in flight during layer 1 (k_dec_a: 244 VGPRs beside its prefetch).
template <class Pix>
__device__ __forceinline__ void wino_l1_rows(f32x16 (&out)[2][2], const float4* __restrict__ U, const float4* sm, const int h,
                                             const int mt_, Pix pix) {
    const unsigned ln = (threadIdx.x & 63u) * 16u;
    const __amdgpu_buffer_rsrc_t ur = wrsrc(U);
    int mt = mt_; asm volatile("" : "+s"(mt));              // (laundered per call, as in wino_l1)
    auto ufrag = [&](int a, int b, int kc) { return wfrag(ur, ln, (size_t)(((4 * a + b) * 2 + mt) * 8 + kc) * 64); };
    auto bases = [&](int a, int (&pb)[8]) {                 // d[i0][0..3], d[i1][0..3] of xi row a
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) { pb[jj] = pix(wino_i0(a), jj); pb[4 + jj] = pix(wino_i1(a), jj); }
    };
    float4 aq[4], raw[8];                                   // the A fragments (one chunk of the four xi ahead) and the raw pixels of the next chunk
    int pb[8];
#pragma unroll
    for (int b = 0; b < 4; ++b) aq[b] = ufrag(0, b, 0);
    bases(0, pb);
#pragma unroll
    for (int q = 0; q < 8; ++q) raw[q] = sm[pb[q] + h];
    f32x16 xacc[4];
    const f32x16 zero = {};
    auto xi_row = [&](int a, auto mask) {
        const float s1 = wino_s1(a);
        const int an = a + 1 < 4 ? a + 1 : a;              // the next xi row (the last one re-reads its own fragments: never used)
#pragma unroll
        for (int kc = 0; kc < 8; ++kc) {
            float4 av[4], col[4], v[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) { av[b] = aq[b]; aq[b] = kc < 7 ? ufrag(a, b, kc + 1) : ufrag(an, b, 0); }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) col[jj] = fma4(s1, raw[4 + jj], raw[jj]);
#pragma unroll
            for (int b = 0; b < 4; ++b) v[b] = fma4(wino_s1(b), col[wino_i1(b)], col[wino_i0(b)]);
            if (kc == 7) bases(an, pb);
#pragma unroll
            for (int q = 0; q < 8; ++q) raw[q] = sm[pb[q] + (kc < 7 ? 2 * (kc + 1) : 0) + h];
            prio_matrix();
            __builtin_amdgcn_sched_barrier(0);              // keep the prefetch loads AHEAD of this chunk's MFMAs
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                f32x16& x = xacc[b];
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b].x, v[b].x, kc == 0 ? zero : x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b].y, v[b].y, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b].z, v[b].z, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_32x32x2f32(av[b].w, v[b].w, x, 0, 0, 0);
                if (b < 3) __builtin_amdgcn_sched_barrier(0);      // xi by xi (hipcc deals the four chains round-robin otherwise: every accumulator's last MFMA among the chunk's last four)
            }
            prio_nonmatrix();
        }
        // the row's transforms in ascending xi, each behind the one before it: xi (a, 0)'s accumulator has been complete for twelve
        // MFMAs, and by the time xi (a, 3)'s is read its last MFMA has left the pipe (the barriers keep hipcc from starting at the far end)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            wino_otrans<2, 0, decltype(mask)::value>(out, a, b, xacc[b]);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    xi_row(0, std::integral_constant<int, 1>{});           // a = 0: row 0 only; a = 1, 2: both; a = 3: row 1 only
#pragma unroll 1
    for (int a = 1; a < 3; ++a) xi_row(a, std::integral_constant<int, 3>{});
    xi_row(3, std::integral_constant<int, 2>{});
}
// ---------------------------------------------------------------------------------------------------------
// Layer 2 (ConvTranspose2d(64,64,3,s2,p1,op1)) by F(2, 2) (the table and the six-group schedule at the top of this file) on
// v_mfma_f32_16x16x4_f32: one call contracts a tile of 16 output channels (M) x 16 blocks of 2 x 2 layer-1 pixels (N, lane n = lane & 15)
// over the 64 input channels (K = 4 per instruction: lane group g = lane >> 4 supplies channel quad 4 kc + g of chunk kc, so one
// ds_read_b128 feeds four MFMAs).  acc[4 orow + ocol] holds channels 16 ct + 4 g + 0..3 of output pixel (orow, ocol) of the lane's block.
// The association of every output element, the same in k_dec_a and k_dec_a_s: the bias; then groups 0..5 in order, in each the direct
// chains (channel chunks 0..3, four channels per MFMA) straight into their output, then the temporaries added in chain order.
// nb: LDS float4 indices (the lane's quad g included) of the block's 3 x 3 pixel neighbourhood: pixel (i, jj), i, jj < 2, at
// xb + (16 i + jj) DA_PS; column 2 of row i at c2[i]; row 2, column jj < 2, at r2 + jj DA_PS (the callers point x_2 beyond the last
// row / column at zero pixels).  With the lane order n = 8 (block row & 1) + block column the lanes that one ds_read_b128 pass serves
// ({0-3, 12-15} of a lane group and {4-11} of the next: pixels at a stride of two, quads at distance one) hit 16 distinct bank quads.
// U: packed [16 matrices][4 channel tiles][4 chunks][64 lanes][4] (engine_weights.hip); wr: the resource based at this channel tile; dn: distance
// to the tile contracted next (0 or 1), whose first fragments are requested behind this tile's last ones.  aq: the fragments of the
// tile's first F22_PD steps on entry (f22_l2_first), of the next tile's on exit.
// ---------------------------------------------------------------------------------------------------------
struct F22Nb { int xb, c2[3], r2; };
// the neighbourhood of the block at xb (the lane's quad included) in block column bv; zq: a zero pixel (quad included), the x_2 of the last
// block column and of block row bu = 7 (an image with a row of zeros below it passes bu = 0: row 2 is then a row like any other)
__device__ __forceinline__ F22Nb f22_nb(const int xb, const int zq, const int bv, const int bu) {
    F22Nb nb;
    nb.xb = xb;
    nb.c2[0] = bv == 7 ? zq : xb + 2 * DA_PS;
    nb.c2[1] = bv == 7 ? zq : xb + 18 * DA_PS;
    nb.c2[2] = (bv == 7 || bu == 7) ? zq : xb + 34 * DA_PS;
    nb.r2 = bu == 7 ? zq : xb + 32 * DA_PS;
    return nb;
}
__device__ __forceinline__ f32x4 f22_wfrag(const __amdgpu_buffer_rsrc_t wr, const unsigned ln, int ct, int m, int kc) {
    return __builtin_bit_cast(f32x4, wfrag(wr, ln + (unsigned)kc * 1024u, (size_t)(m * 4 + ct) * 256));      // kc: the load's immediate offset
}
constexpr int F22_PD = 2;                              // A-fragment prefetch distance in steps (16 - 20 MFMAs each; fragments come from L2)
// the fragments of steps 0 .. F22_PD - 1 of the tile dn tiles behind wr's
__device__ __forceinline__ void f22_l2_first(f32x4 (&aq)[F22_PD][5], const __amdgpu_buffer_rsrc_t wr, const int dn, const unsigned ln) {
    static_for<F22_PD>([&](auto p) {
        static_for<w3_nch(p >> 2)>([&](auto c) { aq[p][c] = f22_wfrag(wr, ln, dn, w3_mat(w3_prod(p >> 2, c)), p & 3); });
    });
}
// LATE: k_dec_ab alone.  k_dec_a and k_dec_a_s keep the adds behind the group's last MFMA: beside their live prefetch of the next
// image the later placement takes k_dec_a to 256 VGPRs and spills.  Plain vector adds and subtracts (a measured choice).
template <bool LATE = false>
__device__ __forceinline__ void f22_l2(f32x4 (&acc)[16], f32x4 (&aq)[F22_PD][5], const __amdgpu_buffer_rsrc_t wr, const int dn,
                                       const unsigned ln, const f32x4 bias4, const f32x4* smv, const F22Nb& nb) {
    auto px = [&](int i, int jj, int kc) -> f32x4 {
        return smv[(jj == 2 ? nb.c2[i] : (i == 2 ? nb.r2 + jj * DA_PS : nb.xb + (16 * i + jj) * DA_PS)) + 4 * kc];
    };
    f22_contract<F22_PD, LATE, false, true>(acc, aq, bias4, [&](int m, int kc, bool next) { return f22_wfrag(wr, ln, next ? dn : 0, m, kc); }, px, [](auto) {});
}
// ReLU + the tile's y2 stores.  y2 is [parity][8 channel groups][16 x 16 positions][8 channels]: outputs (orow, c) and (orow, c + 2) of a
// block are neighbouring positions of one parity, and lane groups g, g ^ 1 are the two halves of one 8-channel group.  One
// v_permlane32_swap per register pair gives lanes 0-31 the pair's values of channel group 2 ct (lanes 32-63: the next position) and
// the second register those of channel group 2 ct + 1, so that a store instruction writes a block row's 16 positions x 32 bytes as
// one 512-byte run (two block rows: two runs).  yr: the image; yoff: byte offset of (block row, block column, g) inside a plane,
// ((32 bu + 2 bv + (g >> 1)) 2 + (g & 1)) 16; on: lanes that store (the swaps run on every lane).
__device__ __forceinline__ void f22_l2_store(f32x4 (&acc)[16], const __amdgpu_buffer_rsrc_t yr, const unsigned yoff, const int ct, const bool on) {
#pragma unroll
    for (int orow = 0; orow < 4; ++orow)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            u32x4 lo, hi;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned x0 = __builtin_bit_cast(unsigned, relu_nan(acc[4 * orow + c][e]));
                const unsigned x1 = __builtin_bit_cast(unsigned, relu_nan(acc[4 * orow + c + 2][e]));
                const auto sw = __builtin_amdgcn_permlane32_swap(x0, x1, false, false);
                lo[e] = sw[0]; hi[e] = sw[1];
            }
            const unsigned so = (unsigned)(((2 * (orow & 1) + c) * 4096 + 2 * ct * 512 + (orow >> 1) * 32) * 16);
            if (on) {
                __builtin_amdgcn_raw_buffer_store_b128(lo, yr, yoff, so, 0);
                __builtin_amdgcn_raw_buffer_store_b128(hi, yr, yoff, so + 512u * 16u, 0);
            }
        }
}

// Four waves per image (256 VGPRs, 2 waves per SIMD).  Layer 1: 32 channels x 32 Winograd tiles per wave; layer 2: four passes of 16 channels
// x 16 blocks (block rows 2 w, 2 w + 1) per wave.
// k_dec_ab: a by-value kernel argument read from the kernel-argument segment again (scalar loads), through a laundered pointer.  Both
// bodies use about a hundred SGPRs on their own; the arguments of the one loaded once and kept through the other are SGPR spills.
template <class T>
__device__ __forceinline__ T karg_reload(const int kp_lo, const int kp_hi, const size_t offset) {      // kp_*: the segment's address, parked (vpark)
    const unsigned long long base = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(kp_hi) << 32) | (unsigned)__builtin_amdgcn_readfirstlane(kp_lo);
    const __attribute__((address_space(4))) char* p = (const __attribute__((address_space(4))) char*)base + offset;
    T t;
    __builtin_memcpy(&t, reinterpret_cast<const __attribute__((address_space(4))) T*>(p), sizeof(T));      // (T's alignment: scalar loads)
    return t;
}

// k_dec_ab: a uniform value parked in a vector register between its uses (vpark), read back as a scalar where it is needed (vscalar): both
// bodies are short of SGPRs, not of VGPRs, and a scalar that lives through a whole image with two uses is better kept out of their way.
__device__ __forceinline__ int vpark(int x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ int vscalar(int x) { return __builtin_amdgcn_readfirstlane(x); }

// pieces lo .. hi - 1 of thread (wave w, lane index tl)'s 16 float4s of image pimg: buffer loads (uniform image base, one lane offset)
__device__ __forceinline__ void dec_a_load_x4(f32x4 (&pf)[16], const float* x4, const int pimg, const int w, const int tl, const int lo, const int hi) {
    const __amdgpu_buffer_rsrc_t xr = wrsrc(x4 + (size_t)pimg * 16384);
#pragma unroll
    for (int it = 0; it < 16; ++it)     // (it & 3: the load's immediate offset; three scalar offsets instead of fifteen)
        if (it >= lo && it < hi) pf[it] = __builtin_bit_cast(f32x4, wfrag(xr, (unsigned)(w * 16384 + (tl & 63) * 16 + (it & 3) * 1024), (size_t)(it >> 2) * 256));
}

// The persistent image loop of k_dec_a, shared with k_dec_ab (FUSED), which carries every image on through k_dec_b4's body: there y2 goes to the
// workgroup's own slot a.y2 + blockIdx.x * 64 Ki floats, tail(img, nimg, pf) runs behind a live image's y2 stores (it requests the next image's
// x4 itself) and, as its LDS aliases this one's, the zero row is written again for every image.
template <bool FUSED, class Tail>
__device__ __forceinline__ void dec_a_loop(const DecAArgs& a_, float4* const sm, Tail&& tail, const int kp_lo = 0, const int kp_hi = 0) {
    const DecAArgs& a = a_;
    constexpr int NTHR = 256;
    constexpr int NPH = 2048 / NTHR;                  // float4s per thread of each image half
    constexpr int NPE = 8;                            // float4s of the next image requested ahead of layer 2, the others behind its last contraction
    // sm: [273 pixels][DA_PS slots]; pixels 256 .. 272 = zeros
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w_ = __builtin_amdgcn_readfirstlane(tid >> 6);

    if ((int)blockIdx.x >= a.rows) return;
    // Image schedule: the first two images of a workgroup are static (blockIdx, blockIdx + grid), the rest are claimed from a
    // ticket counter.  The two workgroups of a CU do not run at the same speed (the older one wins the MFMA arbitration,
    // ~300k vs ~365k cycles per image), so a static stride leaves the younger one alone -- at half the CU's throughput -- for
    // the last ~18 % of the kernel.  Tickets are fetched two images ahead by thread 0 and handed over through LDS.
    int* const slot = reinterpret_cast<int*>(sm + DA_BIAS + 32);
    if (tid == 0) slot[0] = 2 * (int)gridDim.x + atomicAdd(a.queue, 1);
    int nimg = (int)blockIdx.x + (int)gridDim.x;
    // next image, in flight during compute
    f32x4 pf[2 * NPH];
    f32x4* smv = reinterpret_cast<f32x4*>(sm);
    {
        const f32x4* X = reinterpret_cast<const f32x4*>(a.x4) + (size_t)blockIdx.x * 4096;
#pragma unroll
        for (int it = 0; it < 2 * NPH; ++it) pf[it] = X[w_ * 1024 + it * 64 + lane];      // wave w: pixels 64 w .. 64 w + 63 (16 KiB contiguous)
    }
    if constexpr (!FUSED)
        for (int i = tid; i < 17 * DA_PS; i += NTHR) sm[256 * DA_PS + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    // biases live in LDS: a global bias load inside an epilogue forces s_waitcnt vmcnt(0), i.e. waits for every store
    // issued before it (vmcnt retires in order) and serialises the whole store stream
    if (tid < 16) sm[DA_BIAS + tid] = reinterpret_cast<const float4*>(a.b1)[tid];
    else if (tid < 32) sm[DA_BIAS + tid] = reinterpret_cast<const float4*>(a.b2)[tid - 16];

    const int rows_v = FUSED ? vpark(a_.rows) : 0, bx_v = FUSED ? vpark((int)blockIdx.x) : 0;
    if constexpr (FUSED) nimg = vpark(nimg);
    for (int img = FUSED ? vpark((int)blockIdx.x) : (int)blockIdx.x; (FUSED ? vscalar(img) : img) < (FUSED ? vscalar(rows_v) : a_.rows);) {
        // (k_dec_ab: the arguments read again for every image, see karg_reload; they are the first member of its argument struct)
        DecAArgs ai;
        if constexpr (FUSED) ai = karg_reload<DecAArgs>(kp_lo, kp_hi, 0);
        const DecAArgs& a = FUSED ? ai : a_;
        const float4* W1 = reinterpret_cast<const float4*>(a.w1);
        const float4* W2 = reinterpret_cast<const float4*>(a.w2);
        // stage the 16x16x64 input image (64 KiB) into the swizzled LDS layout
        // per-image laundering of the thread index: stops hipcc hoisting ~40 loop-invariant staging / prefetch addresses out of
        // the image loop, which pushed the kernel over 256 VGPRs (spill reloads carry s_waitcnt vmcnt(0): they serialised
        // the prefetch loads and waited for every outstanding y2 store)
        int tl_ = tid; asm volatile("" : "+v"(tl_));
        const int j = tl_ & 31, h = (tl_ >> 5) & 1;
        const int w = FUSED ? __builtin_amdgcn_readfirstlane(tl_ >> 6) : w_;      // (k_dec_ab: no scalar multiple of it kept from image to image)
        // a dead row of the call (efe_rows.mask) keeps the schedule -- barriers, ticket, the next image's prefetch -- and skips the work
        // (k_dec_ab: made a scalar, so that the branches on it are uniform ones -- under a lane mask, the next image's x4 requested in the
        // dead branch would stay live through both bodies of the live one)
        const bool live = FUSED ? __builtin_amdgcn_readfirstlane((int)row_live(a.live, vscalar(img))) != 0 : row_live(a.live, img);
        if (live) {   // pixel 64 w + 4 it + (lane >> 4), quad lane & 15: one address register, immediate offsets
            const int sbase = (64 * w + ((tl_ >> 4) & 3)) * DA_PS + (tl_ & 15);
#pragma unroll
            for (int it = 0; it < 2 * NPH; ++it) smv[sbase + it * 4 * DA_PS] = pf[it];
        }
        if constexpr (FUSED)
            for (int i = tl_; i < 17 * DA_PS; i += NTHR) sm[256 * DA_PS + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int nnimg = slot[0];                   // the image after nimg (written one iteration ago)
        int ticket = 0;
        if ((FUSED ? tl_ : tid) == 0) ticket = 2 * (int)gridDim.x + atomicAdd(a.queue, 1);     // lands during the layer-1 contraction
        // ---------------- layer 1 (Winograd F(2x2, 3x3), see wino_l1): wave w owns channels 32 (w >> 1) .. + 31 of the 32 tiles
        // 32 (w & 1) .. + 31 (tile n = 8 ty + tx: tile rows 4 (w & 1) .. + 3), lane j = tile
        const int l1mt = w >> 1, l1n = 32 * (w & 1) + j;
        const int l1y = 2 * (l1n >> 3) - 1, l1x = 2 * (l1n & 7) - 1;      // the tile's input corner (may be -1: padding)
        if (live) {     // (workgroup-uniform: both branches pass the same barriers; the outputs live in this branch alone)
            f32x16 l1o[2][2];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {           // the outputs start at the bias (register e holds channel 32 mt + (e & 3) + 8 (e >> 2) + 4 h)
                const float4 bb = sm[DA_BIAS + l1mt * 8 + 2 * g4 + h];
#pragma unroll
                for (int rc = 0; rc < 4; ++rc) { l1o[rc >> 1][rc & 1][4 * g4] = bb.x; l1o[rc >> 1][rc & 1][4 * g4 + 1] = bb.y; l1o[rc >> 1][rc & 1][4 * g4 + 2] = bb.z; l1o[rc >> 1][rc & 1][4 * g4 + 3] = bb.w; }
            }
            auto l1pix = [&](int i, int jj) {
                const int y = l1y + i, x = l1x + jj;
                return ((unsigned)y < 16u && (unsigned)x < 16u ? y * 16 + x : 256) * DA_PS;
            };
            if constexpr (FUSED) wino_l1_rows(l1o, W1, sm, h, l1mt, l1pix);
            else wino_l1<2, 0>(l1o, W1, sm, h, l1mt, l1pix);
            __syncthreads();            // every wave is done reading the input image (and slot[0])
            if ((FUSED ? tl_ : tid) == 0) slot[0] = ticket;
            // bias + ReLU, written back IN PLACE as the input image of layer 2 (same padded layout)
#pragma unroll
            for (int rc = 0; rc < 4; ++rc) {
                const int pix = (l1y + 1 + (rc >> 1)) * 16 + l1x + 1 + (rc & 1);
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x16& o = l1o[rc >> 1][rc & 1];
                    float4 v;
                    v.x = relu_nan(o[4 * g4 + 0]); v.y = relu_nan(o[4 * g4 + 1]);
                    v.z = relu_nan(o[4 * g4 + 2]); v.w = relu_nan(o[4 * g4 + 3]);
                    sm[pix * DA_PS + l1mt * 8 + 2 * g4 + h] = v;
                }
            }
        } else {
            __syncthreads();
            if ((FUSED ? tl_ : tid) == 0) slot[0] = ticket;
        }
        __syncthreads();
        // ---------------- layer 2 (stride 2) by F(2, 2), see f22_l2: wave w owns block rows 2 w, 2 w + 1 (lane n = 8 (row & 1) + block
        // column) and walks the four 16-channel tiles; the last block row reads its x_2 from the zero row, the last block column from pixel 256
        {
            // (the thread index laundered again: the lane constants of layer 2 must not be formed ahead of layer 1, which has no registers for them)
            int t2_ = tid; asm volatile("" : "+v"(t2_));
            const int n = t2_ & 15, g = (t2_ >> 4) & 3;
            const int bu = 2 * w + (n >> 3), bv = n & 7;
            const F22Nb nb = f22_nb((32 * bu + 2 * bv) * DA_PS + g, 256 * DA_PS + g, bv, 0);      // (0: block row 7 reads the zero row, at the banks of a real row)
            const unsigned ln = (unsigned)(t2_ & 63) * 16u;
            const unsigned yoff = (unsigned)(((32 * bu + 2 * bv + (g >> 1)) * 2 + (g & 1)) * 16);
            const __amdgpu_buffer_rsrc_t yr = wrsrc(a.y2 + (size_t)(FUSED ? vscalar(bx_v) : __builtin_amdgcn_readfirstlane(img)) * (32 * 32 * 64));   // (uniform: img comes from LDS)
            // the next image: NPE float4s are requested ahead of the four passes, the others behind the last contraction (layer 1 has no
            // registers for any, a pass of layer 2 for half; the last tile's stores and the image barrier cover a part of that latency, the
            // CU's other workgroup the rest).  Buffer loads (uniform image base, one lane offset; the image is clamped on the last pass:
            // unconditional loads keep pf[] in registers)
            auto load_next = [&](const int lo, const int hi) {
                const int pimg = __builtin_amdgcn_readfirstlane(nimg < a.rows ? nimg : img);
                dec_a_load_x4(pf, a.x4, pimg, w, t2_, lo, hi);
            };
            if (live) {
                f32x4 aq[F22_PD][5], acc2[16];
                f22_l2_first(aq, wrsrc(W2), 0, ln);
                if constexpr (!FUSED) load_next(0, NPE);
#pragma unroll 1
                for (int ct = 0; ct < 4; ++ct) {
                    const f32x4 bias4 = smv[DA_BIAS + 16 + 4 * ct + g];
                    f22_l2<FUSED>(acc2, aq, wrsrc(W2 + ct * 256), ct < 3 ? 1 : 0, ln, bias4, smv, nb);
                    if (ct < 3) f22_l2_store(acc2, yr, yoff, ct, true);
                }
                if constexpr (!FUSED) load_next(NPE, 2 * NPH);
                f22_l2_store(acc2, yr, yoff, 3, true);
                if constexpr (FUSED) tail(img, nimg, pf);      // (in this branch: every path through the image then requests pf anew)
            } else {
                load_next(0, 2 * NPH);
            }
        }
        __syncthreads();                // every wave is done reading layer-1's image before the next one overwrites it
        img = nimg; nimg = FUSED ? vpark(nnimg) : nnimg;      // (k_dec_ab: the schedule lives in vector registers, read as scalars where used)
    }
}

__global__ void __launch_bounds__(256, 2) k_dec_a(const DecAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 sm[];
    dec_a_loop<false>(a, sm, [](int, int, f32x4 (&)[16]) {});
}

// ---------------------------------------------------------------------------------------------------------
// k_dec_a_s: the same two layers for SMALL launches (<= 128 images: the one-episode planner), one image over EIGHT workgroups.
// Workgroup (image, p) owns the layer-2 input rows 2p, 2p + 1 (output rows 4p .. 4p + 3): it computes layer 1 for rows 2p .. 2p + 3
// (the stride-2 layer reads one row below its own) from the input rows 2p - 1 .. 2p + 4, keeps them in LDS and contracts layer 2
// for its row pair.  Every output element sees the operations of k_dec_a in the same order (layer 1: bias as start value, then xi
// ascending, each xi-GEMM over channel blocks 0..7; layer 2: bias, taps, channel blocks 0..7): bit-identical results.
// Waves: layer 1: (feature tile mt = w >> 1, output row r = w & 1 of the 16 Winograd tiles); layer 2: (mt = w >> 1, parities {(0,0), (1,1)} or {(0,1), (1,0)}).
// ---------------------------------------------------------------------------------------------------------
constexpr int DAS_IN = 6 * 16;                      // staged input pixels (+ a zero pixel)
constexpr int DAS_L1 = 4 * 16;                      // layer-1 pixels kept (+ two zero pixels)
constexpr int DAS_BIAS = (DAS_IN + 1 + DAS_L1 + 2) * DA_PS;
constexpr size_t DAS_LDS_BYTES = (DAS_BIAS + 32) * sizeof(float4);
__global__ void __launch_bounds__(256, 2) k_dec_a_s(const DecAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 sm[];
    float4* sin = sm;                                // [6 rows][16][DA_PS], pixel 96 = zeros
    float4* sl1 = sm + (DAS_IN + 1) * DA_PS;         // [4 rows][16][DA_PS], pixels 64, 65 = zeros
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    const int img = blockIdx.x >> 3, p = blockIdx.x & 7;
    if (!row_live(a.live, img)) return;
    const float4* W1 = reinterpret_cast<const float4*>(a.w1);
    const float4* W2 = reinterpret_cast<const float4*>(a.w2);
    {   // stage input rows 2p - 1 .. 2p + 4 (rows outside the image are zeros): 1536 float4, six per thread
        const float4* X = reinterpret_cast<const float4*>(a.x4) + (size_t)img * 4096;
        const int c4 = tid & 15, px0 = tid >> 4;
        float4 v[6];
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int pix = px0 + 16 * it, lr = pix >> 4, y = 2 * p - 1 + lr;
            v[it] = (y >= 0 && y < 16) ? X[(y * 16 + (pix & 15)) * 16 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int it = 0; it < 6; ++it) sin[(px0 + 16 * it) * DA_PS + c4] = v[it];
    }
    if (tid < 16) sin[DAS_IN * DA_PS + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 2 * DA_PS) sl1[DAS_L1 * DA_PS + tid] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < 16) sm[DAS_BIAS + tid] = reinterpret_cast<const float4*>(a.b1)[tid];
    else if (tid < 32) sm[DAS_BIAS + tid] = reinterpret_cast<const float4*>(a.b2)[tid - 16];
    __syncthreads();
    const int mt = w >> 1;
    {   // ---- layer 1 (Winograd, wino_l1) for the 16 tiles of tile rows p, p + 1 (image rows 2p .. 2p + 3): wave w owns output row
        // r = w & 1 of every tile (lanes j and j + 16 hold the same tile; the upper half is not stored)
        const int r = w & 1, n = j & 15;
        const int ly = 2 * (n >> 3) - 1, lx = 2 * (n & 7) - 1;          // the tile's input corner, in staged rows (2p - 1 = row 0) + 1
        f32x16 o[1][2];
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const float4 bb = sm[DAS_BIAS + mt * 8 + 2 * g4 + h];
#pragma unroll
            for (int c = 0; c < 2; ++c) { o[0][c][4 * g4] = bb.x; o[0][c][4 * g4 + 1] = bb.y; o[0][c][4 * g4 + 2] = bb.z; o[0][c][4 * g4 + 3] = bb.w; }
        }
        auto pix = [&](int i, int jj) {
            const int sy = ly + 1 + i, x = lx + jj, y = 2 * p - 1 + sy;
            return ((unsigned)y < 16u && (unsigned)x < 16u ? sy * 16 + x : DAS_IN) * DA_PS;
        };
        if (r) wino_l1<1, 1>(o, W1, sin, h, mt, pix);
        else wino_l1<1, 0>(o, W1, sin, h, mt, pix);
        if (j < 16)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                float4 v;
                v.x = relu_nan(o[0][c][4 * g4 + 0]); v.y = relu_nan(o[0][c][4 * g4 + 1]);
                v.z = relu_nan(o[0][c][4 * g4 + 2]); v.w = relu_nan(o[0][c][4 * g4 + 3]);
                sl1[((ly + 1 + r) * 16 + lx + 1 + c) * DA_PS + mt * 8 + 2 * g4 + h] = v;
            }
    }
    __syncthreads();
    // ---- layer 2 (F(2, 2), f22_l2) for the block row p (input rows 2p, 2p + 1, x_2 from row 2p + 2): wave w contracts channel tile w.
    // A block row has 8 blocks: lanes n >= 8 repeat the blocks of lanes n - 8 and are not stored (half of the MFMA tile is idle)
    {
        const int n = lane & 15, g = lane >> 4, bv = n & 7;
        const F22Nb nb = f22_nb(2 * bv * DA_PS + g, DAS_L1 * DA_PS + g, bv, p);
        const unsigned ln = (unsigned)lane * 16u;
        const unsigned yoff = (unsigned)(((32 * p + 2 * bv + (g >> 1)) * 2 + (g & 1)) * 16);
        const __amdgpu_buffer_rsrc_t yr = wrsrc(a.y2 + (size_t)img * (32 * 32 * 64));
        const __amdgpu_buffer_rsrc_t wr = wrsrc(W2 + w * 256);
        f32x4 aq[F22_PD][5], acc2[16];
        f22_l2_first(aq, wr, 0, ln);
        const f32x4 bias4 = reinterpret_cast<const f32x4*>(sm)[DAS_BIAS + 16 + 4 * w + g];
        f22_l2(acc2, aq, wr, 0, ln, bias4, reinterpret_cast<const f32x4*>(sl1), nb);
        f22_l2_store(acc2, yr, yoff, w, n < 8);
    }
}

constexpr size_t DA_LDS_BYTES = (DA_BIAS + 33) * sizeof(float4);
int init_dec_b_kernels();
// kernels that need more than the default 64 KiB of dynamic LDS: set once per device (called from efe_create)
int init_decoder_kernels() {
    if (hipFuncSetAttribute((const void*)k_dec_a, hipFuncAttributeMaxDynamicSharedMemorySize, DA_LDS_BYTES) != hipSuccess) return 1;
    if (hipFuncSetAttribute((const void*)k_dec_a_s, hipFuncAttributeMaxDynamicSharedMemorySize, DAS_LDS_BYTES) != hipSuccess) return 1;
    return init_dec_b_kernels();
}

void launch_dec_a(const DecAArgs& a, hipStream_t st) {
    if (a.parts == 8) {                                   // small launch: an image over eight workgroups
        hipLaunchKernelGGL(k_dec_a_s, dim3(a.rows * 8), dim3(256), DAS_LDS_BYTES, st, a);
        return;
    }
    const size_t lds = DA_LDS_BYTES;
    const int grid = a.rows < 512 ? a.rows : 512;         // persistent: 2 workgroups per CU
    hipLaunchKernelGGL(k_dec_a, dim3(grid), dim3(256), lds, st, a);
}


// k_dec_b4: ConvT3 + ReLU + ConvT4 + sigmoid + the per-image sums.  One workgroup (4 waves) per image walks 8 strips of SR = 4 input
// rows (+ 1 halo row) staged in LDS.  Wave w owns block row u = w >> 1 of the strip (input rows 2u .. 2u + 2, y3 rows 4u .. 4u + 3) and
// output channels 16 hf .. + 15, hf = w & 1, on v_mfma_f32_16x16x4_f32: M = 16 channels, N = the 16 block columns (lane v = lane & 15),
// K = 4 channels per instruction (lane group g = lane >> 4 supplies channel quad 4 kc + g of chunk kc; one ds_read_b128 feeds 4 MFMAs).
// 25 products x 16 instructions = 400 x 32 cycles per strip and wave (the direct form on 32x32x2: 288 x 64).  The accumulators: 16 output
// positions (orow, ocol) of the block x f32x4 (channels 16 hf + 4 g + r) = 64 VGPRs.
// Staged pixels are [row][33 columns][17 float4 slots] (column 32 = zeros, the x2 of the last block column): a view's lanes read 16 pixels
// at a 2-pixel stride, lane groups g and g + 1 (one ds_read_b128 lane group) quads of odd distance, so the 16 lanes of a lane group hit 16
// distinct bank quads (even pixel offsets for one, odd for the other).
// The 32 -> 1 conv: per output position, 4 v_mfma_f32_16x16x4_f32 on the ReLU'd accumulators with A rows = taps 4 kh + kw (9 of 16 used):
// lane group kh then holds the three kw taps of its block column's four pixels, and the horizontal part of the 3 x 3 sum,
//     H[kh][r][ow] = sum_kw T[kh,kw][r][ow + 1 - kw],
// is formed in registers (the neighbours across a block edge are one DPP row shift away; the shifts' zeros are the image edges).  Each
// channel half writes its H planes (one ds_write_b128 per lane and y3 row) to an LDS ring; the gather adds the halves.
// Deferred gather: the gather of a strip (sigmoid + entropy / reward terms of its 2 SR output rows) runs DURING THE NEXT STRIP'S
// CONTRACTION, in pieces between its MFMA groups (a wave's VALU instructions issue in the shadow of the other wave's MFMAs).  The H-plane
// ring holds 4 SR + 2 rows so that the next strip's planes do not overwrite rows still being gathered; the next strip's input is requested
// behind the contraction's last weight-fragment request; the images of the deferred rows are stored after the strip barrier.
// The body of one image (dec_b_image) is shared by k_dec_b4 and by k_dec_ab, which runs it behind k_dec_a's two layers in the same workgroup:
//   sm: the dynamic LDS (input strip + H ring); sb3 [8], sq [4 x 256], sQ [4]: the bias, the parked partial sums and the quarter sums;
//   y2img: the image's y2 (256 KiB); FUSED: sb3 is already loaded (k_dec_ab's tables outlive the image, the zero column and the tap operand
//   do not: the strip area aliases k_dec_a's image and no register survives its layers).
template <int PARTS, bool FUSED>        // PARTS: 1 = one workgroup per image, 4 = four (small launches)
__device__ __forceinline__ void dec_b_image(const DecBArgs& a, float4* const sm, float4* const sb3, float* const sq, float* const sQ,
                                            const int img, const int qtr, const float* const y2img) {
    constexpr int SR = 4, NW = 4, NTHR = 256;
    constexpr int DB_RP = 33;                         // staged pixels per row: 32 columns + a zero column
    constexpr int DB_PS = 17;                         // float4 slots per pixel: 16 channel quads + 1 pad
    constexpr int DB_IN_F4 = (SR + 1) * DB_RP * DB_PS;
    constexpr int DB_YROWS = 4 * SR + 2;
    constexpr int NPF = (SR + 1) * 512 / NTHR;        // 10 float4s of the input strip per thread
    constexpr int NS = 32 / SR;
    float* sH = reinterpret_cast<float*>(sm + DB_IN_F4);       // [ring row][channel half][kh][64 output columns]
    // (k_dec_ab: the thread index laundered per image, so that none of this body's lane constants is formed ahead of k_dec_a's layers)
    int tid = threadIdx.x;
    if constexpr (FUSED) asm volatile("" : "+v"(tid));
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, v = lane & 15;
    const int u = w >> 1, hf = w & 1;
    // Small launches (a.parts == 4: <= 128 images, the one-episode planner's expansions and simulations) split an image over four
    // workgroups: quarter k owns the output rows gathered from strips 2k and 2k + 1 (their H planes need the last y3 row pair of strip
    // 2k - 1, so a quarter contracts that strip again as a halo) -- 3 of the 8 strips of latency instead of 8.  The per-image sum is
    // DEFINED quarter-wise, ((Q0 + Q1) + (Q2 + Q3)) with Q_k reduced over the workgroup on its own, so that one workgroup walking all
    // eight strips (a.parts == 1) and four workgroups walking three each produce the same bits: results stay a function of the noise
    // keys alone, whatever the launch size.
    constexpr int parts = PARTS;
    const int s_lo = parts == 1 ? 0 : (qtr ? 2 * qtr - 1 : 0);          // first strip contracted (the halo strip of quarters 1..3)
    const int s_hi = parts == 1 ? NS : 2 * qtr + 2;

    const int mg = a.m0 + img;
    const int gi = mg / a.rows_per_group;
    const int r = mg - gi * a.rows_per_group;
    int gt, gp, gs;
    group_decode(a.gm, gi, gt, gp, gs);
    const int mode = (gp == 0 && a.reward0) ? 1 : 0;
    const int slot = (gp == 0 && a.store0) ? gt * a.gm.S + gs : -1;
    float* po = (slot >= 0) ? a.po + ((size_t)slot * a.rows_per_group + r) * 4096 : nullptr;
    // (k_dec_ab: the image's scalars that live to its end are kept in vector registers -- k_dec_a's loop state takes their SGPRs)
    int mode_v = mode, mg_v = mg, ri_v = a.reward_intent;
    float* valp = a.val;
    if constexpr (FUSED) { asm volatile("" : "+v"(po)); asm volatile("" : "+v"(valp)); mode_v = vpark(mode_v); mg_v = vpark(mg_v); ri_v = vpark(ri_v); }

    // sq: [quarter][thread], the threads' partial sums of a quarter, reduced once per image
    if constexpr (!FUSED) { if (tid < 8) sb3[tid] = reinterpret_cast<const float4*>(a.b3)[tid]; }
    if (tid < (SR + 1) * 16) sm[((tid >> 4) * DB_RP + 32) * DB_PS + (tid & 15)] = make_float4(0.f, 0.f, 0.f, 0.f);      // the zero column
    // A operand of the 32 -> 1 conv: lane (tap row i = lane & 15 = 4 kh + kw, K row g) holds w4[kh][kw][16 hf + 4 g + rr] in w4a[rr]
    f32x4 w4a;
    {
        const int kh = v >> 2, kw = v & 3;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) w4a[rr] = (kh < 3 && kw < 3) ? a.w4[(3 * kh + kw) * 32 + 16 * hf + 4 * g + rr] : 0.f;
    }

    // the image's y2 through a buffer resource over exactly its 256 KiB: a row below the image is requested at an out-of-range offset
    // and the hardware returns zeros (the halo row of the last strip)
    const __amdgpu_buffer_rsrc_t xr_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(y2img), 0, 32 * 32 * 64 * 4, 0x00020000);
    // (k_dec_ab: the slot's address parked in two vector registers, the resource formed again for every strip)
    const unsigned long long y2a = (unsigned long long)y2img;
    const int y2lo_v = FUSED ? vpark((int)(unsigned)y2a) : 0, y2hi_v = FUSED ? vpark((int)(unsigned)(y2a >> 32)) : 0;
    // packed U fragments [16 matrices][2 channel halves][4 chunks][64 lanes] (engine_weights.hip): the channel half is folded into the base
    const __amdgpu_buffer_rsrc_t wr = wrsrc(a.w3 + (size_t)hf * 4 * 64 * 4);
    const unsigned ln = (unsigned)lane * 16u;
    // (k_dec_ab: the chunk is the load's immediate offset, so that a scalar offset serves four fragments -- with one scalar per fragment
    // hipcc keeps up to 25 of them through the strip loop and spills the gather masks' SGPRs)
    auto wf = [&](int m, int kc, bool) -> f32x4 {       // (f22_contract's form; no step requests another strip's fragments)
        return __builtin_bit_cast(f32x4, FUSED ? wfrag(wr, ln + (unsigned)kc * 1024u, (size_t)(m * 8) * 64) : wfrag(wr, ln, (size_t)(m * 8 + kc) * 64));
    };
    const float D1 = 1.00001f, D0 = 0.00001f;
    float part = 0.f;
    f32x4 pf[NPF];
    f32x4* smv = reinterpret_cast<f32x4*>(sm);
    // Input strip sn (rows SR sn .. SR sn + SR, the last one the halo) in NPF pieces per thread: piece it of thread tl is row it >> 1,
    // 16-byte word (it & 1) 256 + tl of the row's 512.  y2 is [row parity][8 channel groups][16 x 16 positions][2 quads]: the word is
    // position (row >> 1, (tl & 31) >> 1), channel group 8 (it & 1) + (tl >> 5), quad tl & 1 -- a lane offset, a constant per piece and
    // 1 KiB per strip (SR = 4 rows = two rows of positions).  Row 32 (the halo of strip 7) is out of range: the lanes' offsets get bit 31.
    auto prefetch = [&](int sn, int tl) {
        const __amdgpu_buffer_rsrc_t xr = !FUSED ? xr_ : __builtin_amdgcn_make_buffer_rsrc(
            reinterpret_cast<float*>(((unsigned long long)(unsigned)vscalar(y2hi_v) << 32) | (unsigned)vscalar(y2lo_v)), 0, 32 * 32 * 64 * 4, 0x00020000);
        const unsigned lo = (unsigned)(((tl >> 5) * 512 + (tl & 31)) * 16);
        const unsigned lh = lo | (sn == NS - 1 ? 0x80000000u : 0u);
#pragma unroll
        for (int it = 0; it < NPF; ++it) {
            const int rl = it >> 1;
            const unsigned pc = (unsigned)((((rl & 1) * 16 + (it & 1) * 8) * 512 + (rl >> 1) * 32) * 16);
            pf[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr, rl == SR ? lh : lo, pc + (unsigned)sn * 1024u, 0));
        }
    };
    prefetch(s_lo, tid);

    // this lane's block neighbourhood: pixel (2u + i, 2v + jj), quad 4 kc + g at xb + (33 i + jj) * DB_PS + 4 kc (all immediates)
    const int xb = (2 * u * DB_RP + 2 * v) * DB_PS + g;
    auto px = [&](int i, int jj, int kc) -> f32x4 { return smv[xb + (i * DB_RP + jj) * DB_PS + 4 * kc]; };

    // ---- gather of output row oh (lane = column): out = b4 + H[0][oh + 1] + H[1][oh] + H[2][oh - 1] (source row r contributes to
    // oh = r - 1 + kh), the two channel halves added here; split into pieces for the deferred form
    constexpr int RWG = 2 * SR / NW;
    float gh[RWG][6], gpr[RWG];
    // The H ring as byte offsets: a ring row (both channel halves' three planes) is HROW bytes, and a slot offset moves forward by
    // fewer than DB_YROWS rows at a time, so one unsigned minimum wraps it (o - HRING wraps around to a huge value unless o >= HRING).
    constexpr unsigned HROW = 2 * 3 * 64 * sizeof(float), HRING = DB_YROWS * HROW;
    auto ring_fwd = [&](unsigned o, unsigned rows) { o += rows * HROW; const unsigned t = o - HRING; return t < o ? t : o; };
    const float* const sHl = sH + lane;
    // go: ring byte offset of y3 row oh - 1 (the gather's lowest source row); row oh + 1 - kh is 2 - kh ring rows behind it.  gm: all
    // ones where that source row is inside the image, else zero -- the row then contributes +0, whatever its slot holds.
    unsigned gm[RWG][3];
    auto g_load = [&](unsigned go, int q) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const float* hq = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sHl) + (kh == 2 ? go : ring_fwd(go, 2 - kh))) + kh * 64;
            gh[q][2 * kh] = hq[0]; gh[q][2 * kh + 1] = hq[3 * 64];
        }
    };
    auto g_mask = [&](int oh, int q) {
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) gm[q][kh] = (unsigned)(oh + 1 - kh) <= 63u ? ~0u : 0u;
    };
    auto g_sig = [&](int q) {
        float val = a.b4;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
            val = add1(val, __builtin_bit_cast(float, __builtin_bit_cast(unsigned, add1(gh[q][2 * kh], gh[q][2 * kh + 1])) & gm[q][kh]));
        // hardware exp2 / rcp / log2 (v_exp_f32, v_rcp_f32, v_log_f32: 1 ulp each) instead of the libm expansions: ~14 instead of ~60 VALU
        // instructions per pixel, each of which costs ~19 cycles of wave time beside the other wave's MFMA stream; the image stays within
        // 3e-7 of the libm form, the 4096-pixel sums within their own fp32 rounding (tests/test_gpu_parity.py tolerances unchanged)
        gpr[q] = hw_sigmoid(val);
    };
    auto g_term = [&](int oh, int q) {          // branch-free: both forms are evaluated (the reward form is four FMAs), rows above the image add zero
        // (the products are contracted EXPLICITLY: this lambda is inlined at several places -- deferred pieces, strip epilogues, both
        // template instances -- and a row must get the same bits whichever copy evaluates it; left to the compiler, a b - c d may
        // become fma(a, b, -(c d)) in one copy and fma(-c, d, a b) in another)
#pragma clang fp contract(off)
        const float pr = gpr[q];
        const float l1 = hw_log(D1 - pr), l0 = hw_log(D0 + pr);
        const float te = __builtin_fmaf(pr - 1.0f, l1, -(pr * l0));          // -(1 - p) ln((1e-5 + 1) - p) - p ln(1e-5 + p)
        const float tw = reward_term(pr, oh, lane, 64, 64, ri_v);
        const float t = mode_v == 0 ? te : tw;
        part += oh >= 0 ? t : 0.0f;
    };
    auto g_store = [&](int oh, int q) {
        if (po && oh >= 0) {
            int owl = lane; asm volatile("" : "+v"(owl));
            (po + oh * 64)[owl] = gpr[q];
        }
    };

    // a quarter is complete: park the thread's partial sum (one LDS write; the reductions of all quarters run once, behind the last strip)
    auto fold = [&](int k) { sq[k * NTHR + tid] = part; part = 0.f; };
    char* const sHw = reinterpret_cast<char*>(sH + hf * (3 * 64) + g * 64 + 4 * v);     // this lane's place in an H plane of its channel half and tap row
    // The ring's schedule is fixed: the slot of y3 row 2 SR s (this strip's first) advances 2 SR mod DB_YROWS per strip from 0.  hbo is its
    // byte offset; this wave's four write rows (4 u + orow ring rows on) and the six source rows of its deferred gather (rows
    // -(2 SR) - 2 + w + {0, 1, 2, 4, 5, 6} of the previous strip, that is DB_YROWS - 2 SR - 2 + w + ... ring rows on) are wrapped additions from it.
    unsigned hbo = 0;
    const int tl = tid;
    // staging: piece it is row it >> 1, pixel column 2 ((tl & 31) >> 1) + (it & 1), quad 2 (tl >> 5) + (tl & 1) -- one address register,
    // the pieces at immediate offsets (the row below the image arrived as zeros)
    f32x4* const sp = smv + ((tl & 31) >> 1) * (2 * DB_PS) + 2 * (tl >> 5) + (tl & 1);
    for (int s = s_lo; s < s_hi; ++s) {
        const bool gq = parts == 1 ? true : s == 2 * qtr + 1;   // (uniform) the previous strip's rows are this workgroup's to gather
        const int oh0 = 2 * SR * (s - 1) - 1 + w, oh1 = oh0 + NW;         // this wave's two output rows of the previous strip
        const unsigned go0 = ring_fwd(hbo, DB_YROWS - 2 * SR - 2 + w), go1 = ring_fwd(go0, NW);      // rows oh0 - 1, oh1 - 1
        const unsigned hwo = ring_fwd(hbo, 4 * u);
        g_mask(oh0, 0); g_mask(oh1, 1);
        {
#pragma unroll
            for (int it = 0; it < NPF; ++it) sp[((it >> 1) * DB_RP + (it & 1)) * DB_PS] = pf[it];
        }
        f32x4 aq[1][5];                                    // the strip's first weight fragments: in flight across the barrier
#pragma unroll
        for (int c = 0; c < w3_nch(0); ++c) aq[0][c] = wf(w3_mat(w3_prod(0, c)), 0, false);
        __syncthreads();

        // the accumulators start at the layer-3 bias (lane: channels 16 hf + 4 g + 0..3): the C operand of an output's first MFMA, or
        // the first addend of its first temporary
        const f32x4 bias4 = __builtin_bit_cast(f32x4, sb3[4 * hf + g]);
        const f32x4 zero4 = {};
        f32x4 acc[16];
        // ---- contraction (f22_contract: the temporaries added a step later, single-lane adds; the fragment ring one step deep, and
        // dry at the strip's end), with the previous strip's gather, a piece per step
        f22_contract<1, true, true, false>(acc, aq, bias4, wf, px, [&](auto stc) {
            constexpr int ST = decltype(stc)::value;
            if (gq) {
                if constexpr (ST == 0) { g_load(go0, 0); g_load(go1, 1); }
                if constexpr (ST == 2) g_sig(0);
                if constexpr (ST == 5) g_term(oh0, 0);
                if constexpr (ST == 8) g_sig(1);
                if constexpr (ST == 11) g_term(oh1, 1);
            }
        });
        // ---- ReLU, then the 32 -> 1 conv as tap planes (4 v_mfma_f32_16x16x4_f32 per output position, the four columns' chains
        // interleaved) and the horizontal presums of this channel half, one y3 row at a time
        // the next strip's input, behind this strip's last weight-fragment request (k_dec_b4 requests the last strip's own input again,
        // which keeps pf[] unconditional; k_dec_ab does not: its slot is about to be written again)
        if (!(FUSED && s == NS - 1)) prefetch((s < NS - 1) ? s + 1 : NS - 1, tl);
        // Skewed by one row: a row's MFMAs share their scheduling region with the NEXT row's ReLUs and the PREVIOUS row's presums, so
        // that no instruction of the region waits for an MFMA result of the same region (a ReLU sunk in front of the MFMA that reads it
        // costs two hazard wait states, a presum right behind its row's last MFMA ten).  The barrier keeps the ReLUs a block ahead.
        auto relu_row = [&](int orow) {
#pragma unroll
            for (int oc = 0; oc < 4; ++oc)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * orow + oc][e] = relu_nan(acc[4 * orow + oc][e]);
        };
        // T[oc][kw] = tap (kh = g, kw) at column 4 v + oc; H(c) = (T[kw 0] at c + 1 + T[kw 1] at c) + T[kw 2] at c - 1
        auto presum_row = [&](const f32x4 (&T)[4], int orow) {
            f32x4 hv;
            hv[0] = add1(add1(T[1][0], T[0][1]), dpp_shr1_zero(T[3][2]));
            hv[1] = add1(add1(T[2][0], T[1][1]), T[0][2]);
            hv[2] = add1(add1(T[3][0], T[2][1]), T[1][2]);
            hv[3] = add1(add1(dpp_shl1_zero(T[0][0]), T[3][1]), T[2][2]);
            // ring slot of this wave's y3 row 2 SR s + 4 u + orow (uniform: a scalar offset to the lane's address)
            if (g < 3) *reinterpret_cast<f32x4*>(sHw + ring_fwd(hwo, orow)) = hv;
        };
        f32x4 T[2][4];
        relu_row(0);
#pragma unroll
        for (int orow = 0; orow < 4; ++orow) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int oc = 0; oc < 4; ++oc)
                    T[orow & 1][oc] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4a[e], acc[4 * orow + oc][e], e == 0 ? zero4 : T[orow & 1][oc], 0, 0, 0);
            if (orow < 3) relu_row(orow + 1);
            if (orow > 0) presum_row(T[(orow - 1) & 1], orow - 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        presum_row(T[1], 3);
        __syncthreads();
        if (gq) { g_store(oh0, 0); g_store(oh1, 1); }     // the deferred rows' pixels (stores behind the prefetch loads)
        if (parts == 1 && (s == 2 || s == 4 || s == 6)) fold(s / 2 - 1);       // quarter s / 2 - 1 is complete (its second gather ran inside this strip)
        if (s == s_hi - 1) {                                // no successor in this workgroup: the strip's own rows now (and row 63 behind the last strip)
#pragma unroll
            for (int q = 0; q <= RWG; ++q) {
                if (q == RWG && (w != 0 || s != NS - 1)) break;
                const int oh = 2 * SR * s - 1 + q * NW + w;
                g_mask(oh, 0);
                g_load(ring_fwd(ring_fwd(hbo, DB_YROWS - 2), q * NW + w), 0); g_sig(0); g_term(oh, 0); g_store(oh, 0);      // row oh - 1 = 2 SR s - 2 + ...
            }
        }
        hbo = ring_fwd(hbo, 2 * SR);
    }
    fold(parts == 1 ? 3 : 0);
    __syncthreads();
    // Q_k = the xor-tree sum over the 64 lanes of ((wave 0 + wave 1) + (wave 2 + wave 3)) of the parked partials: wave k reduces quarter k
    if (w < (parts == 1 ? 4 : 1)) {
        const float* qk = sq + w * NTHR + lane;
        float val = add1(add1(qk[0], qk[64]), add1(qk[128], qk[192]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o);
        if (lane == 0) sQ[w] = val;
    }
    __syncthreads();
    if (tid == 0) {
        if (parts == 1) valp[mg_v] = add1(add1(sQ[0], sQ[1]), add1(sQ[2], sQ[3]));
        else a.valq[(size_t)mg * 4 + qtr] = sQ[0];          // summed in the same association by the consumer (k_terms)
    }
}

template <int PARTS>
__global__ void __launch_bounds__(256, 2) k_dec_b4(const DecBArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 sm[];
    __shared__ float4 sb3[8];
    __shared__ float sq[4 * 256];
    __shared__ float sQ[4];
    const int img = PARTS == 1 ? (int)blockIdx.x : (int)(blockIdx.x >> 2);
    const int qtr = PARTS == 1 ? 0 : (int)(blockIdx.x & 3);
    if (!row_live(a.live, img)) return;                // a dead row of the call (efe_rows.mask): workgroup-uniform
    dec_b_image<PARTS, false>(a, sm, sb3, sq, sQ, img, qtr, a.y2 + (size_t)img * (32 * 32 * 64));
}

constexpr size_t DB_LDS4D = ((5 * 33) * 17) * sizeof(float4) + 18 * 2 * 3 * 64 * sizeof(float);  // input strip (+ zero column) + H planes per channel half (4 SR + 2 rows)

// ---------------------------------------------------------------------------------------------------------
// k_dec_ab: k_dec_a and k_dec_b4<1> as ONE persistent launch (engine option dec_fuse_ab).  A workgroup takes its images as k_dec_a does
// (two static, then tickets) and carries each one through both bodies: the two layers of dec_a_loop write y2 into the workgroup's own
// 256 KiB slot (a.a.y2 + blockIdx.x * 64 Ki floats, today's layout), and dec_b_image walks its eight strips over that slot.  The hand-over
// is a release / acquire at workgroup scope and nothing more: every wave retires its y2 stores (s_waitcnt vmcnt(0)), then the workgroup
// barrier; the waves share one CU and one vector L1, so no cache is written back or invalidated, and no workgroup ever waits for
// another (the ticket counter stays the only shared word).  Every output element sees the operations of the two kernels in the same order.
// LDS: k_dec_a's region [0, DA_LDS_BYTES) with k_dec_b4's dynamic region aliased onto its image and zero row (the two layers' biases and the
// ticket slot lie behind it and survive), then k_dec_b4's static arrays: 79 024 bytes, two workgroups per CU.  Per image the zero row
// (dec_a_loop), the zero column and the tap operand (dec_b_image) are formed again; the ConvT3 bias is loaded once.
// The next image's x4 is requested behind body b's reduction, the last point of the image: requested anywhere inside the last strip
// (behind its contraction, its tap conv, its barrier or its gather) hipcc spills 89 - 140 VGPRs of it, although fewer than 200 are live
// there.  The image barrier, the zero row and the CU's other workgroup cover the latency; no register holds x4 through a contraction.
// ---------------------------------------------------------------------------------------------------------
constexpr int DAB_SB3 = DA_BIAS + 33, DAB_SQ = DAB_SB3 + 8, DAB_SQQ = DAB_SQ + 256;       // float4 indices behind k_dec_a's region
constexpr size_t DAB_LDS_BYTES = (DAB_SQQ + 1) * sizeof(float4);
static_assert(DB_LDS4D <= DA_BIAS * sizeof(float4), "k_dec_b4's strips and ring must not reach k_dec_a's biases and ticket slot");
static_assert(DAB_LDS_BYTES <= 80 * 1024, "two workgroups of k_dec_ab per CU");
__global__ void __launch_bounds__(256, 2) k_dec_ab(const DecABArgs a) {
    __shared__ __attribute__((aligned(16))) float4 sm[DAB_SQQ + 1];      // static: every region's address is a constant of the instructions
    float4* const sb3 = sm + DAB_SB3;
    float* const sq = reinterpret_cast<float*>(sm + DAB_SQ);
    float* const sQ = reinterpret_cast<float*>(sm + DAB_SQQ);
    if (threadIdx.x < 8) sb3[threadIdx.x] = reinterpret_cast<const float4*>(a.b.b3)[threadIdx.x];      // (read behind the first image's barriers)
    const unsigned long long kp = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    const int kp_lo = vpark((int)(unsigned)kp), kp_hi = vpark((int)(unsigned)(kp >> 32));      // (see karg_reload)
    dec_a_loop<true>(a.a, sm, [&](const int img, const int nimg, f32x4 (&pf)[16]) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's y2 stores have reached the cache the workgroup shares ...
        __syncthreads();                                        // ... and every wave's; layer 2 is done reading the image the strips alias
        const DecBArgs b = karg_reload<DecBArgs>(kp_lo, kp_hi, __builtin_offsetof(DecABArgs, b));
        dec_b_image<1, true>(b, sm, sb3, sq, sQ, __builtin_amdgcn_readfirstlane(img), 0, b.y2 + (size_t)vscalar(vpark((int)blockIdx.x)) * (32 * 32 * 64));
        const DecAArgs an = karg_reload<DecAArgs>(kp_lo, kp_hi, 0);
        int tl = threadIdx.x; asm volatile("" : "+v"(tl));
        const int pimg = __builtin_amdgcn_readfirstlane(nimg < an.rows ? nimg : img);
        dec_a_load_x4(pf, an.x4, pimg, __builtin_amdgcn_readfirstlane(tl >> 6), tl, 0, 16);
    }, kp_lo, kp_hi);
}

int init_dec_b_kernels() {
    if (hipFuncSetAttribute((const void*)k_dec_b4<1>, hipFuncAttributeMaxDynamicSharedMemorySize, DB_LDS4D) != hipSuccess) return 1;
    if (hipFuncSetAttribute((const void*)k_dec_b4<4>, hipFuncAttributeMaxDynamicSharedMemorySize, DB_LDS4D) != hipSuccess) return 1;
    return 0;
}

int dec_ab_grid(int rows, int cap) { const int g = rows < 512 ? rows : 512; return cap > 0 && cap < g ? cap : g; }
void launch_dec_ab(const DecABArgs& a, int grid_cap, hipStream_t st) {
    hipLaunchKernelGGL(k_dec_ab, dim3(dec_ab_grid(a.a.rows, grid_cap)), dim3(256), 0, st, a);      // (its LDS is static)
}

void launch_dec_b(const DecBArgs& a, hipStream_t st) {
    if (a.parts == 4) hipLaunchKernelGGL(k_dec_b4<4>, dim3(a.rows * 4), dim3(256), DB_LDS4D, st, a);
    else hipLaunchKernelGGL(k_dec_b4<1>, dim3(a.rows), dim3(256), DB_LDS4D, st, a);
}

// ---------------------------------------------------------------------------------------------------------
// k_fc4: Linear(256, 64 * base^2) + ReLU + Dropout(0.5) (torchmodel.py:116-118; 16384 features for Dynamic dSprites, 28224 for the
// 84 x 84 geometry), output written NHWC (rows permuted at pack time).  A workgroup stages 64 batch rows x K=256 in swizzled LDS once
// and sweeps steps of 256 features; every wave owns 64 features x 64 rows per step.  Dropout mask = one Philox call per row per 128
// features.  The feature steps (ceil(mtiles / 8)) are dealt to 8 groups of SPG = ceil(steps / 8) consecutive steps (8 x 8 for 16384).
// ---------------------------------------------------------------------------------------------------------
__host__ __device__ inline int fc4_spg(int mtiles) { return ((mtiles + 7) / 8 + 7) / 8; }
template <int NT>          // 32-row batch tiles per workgroup tile: 2 (64 rows), or 1 for launches of <= 32 rows (the one-episode planner's trajectories)
__global__ void __launch_bounds__(256, 2) k_fc4(const GemmArgs a) {
    constexpr int RT = 32 * NT;
    extern __shared__ __attribute__((aligned(16))) float4 sm[];        // [RT rows][64 quads], quad ^= row & 15
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, h = lane >> 5;
    // Persistent, XCD-aware and balanced: workgroup b runs on XCD b % 8 and only ever touches feature group b & 7, so every XCD
    // streams ONE 2 MiB weight slice (L2-resident, 4 MiB per XCD).  The (row tile, feature step) pairs of a feature group are split
    // into equal contiguous ranges over the gridDim/8 workgroups of that XCD: with one workgroup per (row tile, group) the 2400
    // 230-us workgroups of a 19200-row launch ran as 4.7 waves over the 512 slots and the last, 70 %-full wave cost ~8 %.
    const int fgrp = blockIdx.x & 7;
    const int nper = gridDim.x >> 3, k = blockIdx.x >> 3;
    const int SPG = fc4_spg(a.mtiles);
    const int nsteps = ((a.n_pix + RT - 1) / RT) * SPG;                // (row tile, step) pairs of this feature group
    const int q0 = (int)(((long)nsteps * k) / nper), q1 = (int)(((long)nsteps * (k + 1)) / nper);
    f32x4* smv = reinterpret_cast<f32x4*>(sm);
    const float4* Wl = reinterpret_cast<const float4*>(a.Wp);
    auto xaddr = [&](int t, int (&bs)[NT], int (&sw)[NT], int& wt) {
        wt = t;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { bs[nt] = (nt * 32 + j) * 64 + t * 16; sw[nt] = j & 15; }
    };
    int cur_rt = -1;
    uint32_t krow[2] = {0, 0}, kstream[2] = {0, 0}, kstage[2] = {0, 0};
    bool rv[2] = {false, false};
#pragma unroll 1
    for (int q = q0; q < q1; ++q) {
        const int rt = q / SPG, fs = q - rt * SPG;
        const int row0 = rt * RT;
        if (rt != cur_rt) {                                            // (re)stage the 64-row tile: at most twice more than once per workgroup
            if (cur_rt >= 0) __syncthreads();                          // every wave is done reading the previous tile
            cur_rt = rt;
            const f32x4* X = reinterpret_cast<const f32x4*>(a.X);
#pragma unroll
            for (int it = 0; it < 8 * NT; ++it) {
                const int idx = it * 256 + tid;                        // RT rows x 64 quads
                const int r = idx >> 6, c4 = idx & 63;
                const int gr = row0 + r;
                smv[r * 64 + (c4 ^ (r & 15))] = (gr < a.n_pix) ? X[(size_t)gr * 64 + c4] : (f32x4)(0.f);
            }
            __syncthreads();
            // dropout keys of this lane's two rows
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int m = row0 + nt * 32 + j;
                rv[nt] = m < a.n_pix;
                const int mg = a.m0 + (rv[nt] ? m : 0);
                const int g = mg / a.rows_per_group;
                krow[nt] = global_row(a.gm.ids, a.gm.ids_div, mg - g * a.rows_per_group, a.row_offset);
                const uint2 key = group_key(a.gm, g);
                kstream[nt] = key.x; kstage[nt] = key.y;
            }
        }
        const int mt0 = (fgrp * SPG + fs) * 8 + 2 * w;                 // this wave's first 32-feature tile
        if (mt0 >= a.mtiles) continue;                                 // wave-uniform: past the last feature tile (mtiles is even)
        f32x16 acc[2][NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mt][nt][e] = 0.f;
        // the step's bias quads are requested BEFORE the contraction: a load placed between the stores would need
        // s_waitcnt vmcnt(0) and wait for every store ahead of it
        float4 bq[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) bq[mt][g4] = *reinterpret_cast<const float4*>(a.bias + (mt0 + mt) * 32 + 8 * g4 + 4 * h);
        tap_loop<2, NT>(acc, 4, Wl, sm, h, xaddr, DenseWIdx{mt0});
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            if (!rv[nt]) continue;
            const uint4 rnd = noise_words(a.k0, a.k1, a.tag, (uint32_t)((mt0 * 32) >> 7), krow[nt], kstream[nt], kstage[nt]);
            float* yp = a.Y + (size_t)(row0 + nt * 32 + j) * a.ldy;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const int co = (mt0 + mt) * 32 + 8 * g4 + 4 * h;
                    const float4 bb = bq[mt][g4];
                    const uint32_t word = ((co >> 5) & 3) == 0 ? rnd.x : ((co >> 5) & 3) == 1 ? rnd.y : ((co >> 5) & 3) == 2 ? rnd.z : rnd.w;
                    float v[4] = {acc[mt][nt][4 * g4 + 0] + bb.x, acc[mt][nt][4 * g4 + 1] + bb.y,
                                  acc[mt][nt][4 * g4 + 2] + bb.z, acc[mt][nt][4 * g4 + 3] + bb.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = relu_nan(v[e]) * keep2(((word >> ((co + e) & 31)) & 1u));
                    *reinterpret_cast<float4*>(yp + co) = make_float4(v[0], v[1], v[2], v[3]);
                }
        }
    }
}

void launch_fc4(const GemmArgs& a, hipStream_t st) {
    // persistent: 2 workgroups per CU (64 KiB LDS each), 8 feature groups x (up to) 64 workgroups, each with >= 1 (row tile, step) pair
    if (a.n_pix <= 32) {               // one 32-row tile: half the MFMA work of a 64-row tile whose second half would be padding
        const int nsteps = fc4_spg(a.mtiles);
        hipLaunchKernelGGL(k_fc4<1>, dim3(8 * (nsteps < 64 ? nsteps : 64)), dim3(256), 32 * 64 * sizeof(float4), st, a);
        return;
    }
    const int nsteps = ((a.n_pix + 63) / 64) * fc4_spg(a.mtiles);
    const int nper = nsteps < 64 ? nsteps : 64;
    hipLaunchKernelGGL(k_fc4<2>, dim3(8 * nper), dim3(256), 64 * 64 * sizeof(float4), st, a);
}

}  // namespace efe
