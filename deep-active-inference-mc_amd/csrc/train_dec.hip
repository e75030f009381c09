// Backward of the reconstruction loss through the decoder's ConvTranspose2d tail, ModelDown.po_net[12:] (/root/reference/src/torchmodel.py:
// 119-127; the loss: torchloss.py:62), at the Dynamic-dSprites geometry 1 x 64 x 64: the first piece of train_model_down (torchloss.py:90-98).
//     a1 = ConvT(64, 64, s1)(h4)   y1 = relu(a1)      [64][16][16]
//     a2 = ConvT(64, 64, s2)(y1)   y2 = relu(a2)      [64][32][32]
//     a3 = ConvT(64, 32, s2)(y2)   y3 = relu(a3)      [32][64][64]
//     a4 = ConvT(32,  1, s1)(y3)   p  = sigmoid(a4)   [ 1][64][64]
//     nlogpo1_r = -sum_pixels o log(1e-5 + p) + (1 - o) log((1e-5 + 1) - p),     L = scale * sum_r nlogpo1_r
// All layers 3 x 3, padding 1, output_padding stride - 1; W [Cin][Cout][3][3] is read from a raw device copy of the parameters (flat,
// parameters() order, DT_* offsets of kernels.h).  Every activation and gradient is NCHW, the reference's order.
//
// Kernels (one group of at most DEC_TAIL_ROWS rows per pass of launch_dec_tail_group):
//   k_dect_tap<S, CI, CO, HIN, BWD> : tap-GEMM on v_mfma_f32_16x16x4_f32.  One wave = 16 channels x (4 rows x 16 pixels) of the layer's INPUT
//                grid ("virtual" pixels).  Forward (BWD = 0): the 16 pixels are the outputs (S vy + py, S vx + px) of one output parity
//                class (py, px); the class fixes which taps reach it (stride 2: 1, 2, 2 or 4 of the 9) and contracts K = CI per tap;
//                epilogue + bias, ReLU.  Data gradient (BWD = 1): dx[ci][iy][ix] = sum_{co, tap} g[co][S iy - 1 + ky][S ix - 1 + kx] W[ci][co][tap],
//                K = CO per tap, all 9 taps (tap (ky, kx) reads the output pixels of parity (ky - 1, kx - 1) mod S); epilogue: the gate
//                [y_prev > 0] read off the stored activation (none for d_h4).
//   k_dect_out : layer 4 forward (Cout = 1, VALU) + sigmoid -> po1.
//   k_dect_loss: one workgroup per row: nlogpo1 in k_fe_down's expression (loss.hip) and block_sum.h's order over the 4096 pixels, and
//                g4 = -scale (o / (1e-5 + p) - (1 - o) / ((1e-5 + 1) - p)) ((1 - p) p)      finite when p rounds to 0 or 1.
//   k_dect_dx4 : g3 = (sum_tap g4[iy - 1 + ky][ix - 1 + kx] W4[ci][tap]) [y3 > 0]   (VALU, Cout = 1).
//   k_dect_wgrad<S, CI, CO, HIN> : dW[ci][co][tap] = sum_{m, iy, ix} x[m][ci][iy][ix] g[m][co][S iy - 1 + ky][S ix - 1 + kx] (in-range terms):
//                MFMA with K = the positions; one wave owns a 16 ci x 16 co tile for all nine taps (train_conv.h's wgrad_mfma).
//   k_dect_w4  : the 288 weights of layer 4, one workgroup per (ci, slab) (train_conv.h's wgrad_valu).
//   k_conv_bias: db[co] = sum g, one workgroup per (co, slab); defined here, launched by train_enc.hip too (launch_conv_bias).
//   k_slab_sum (train.hip) : gradient = ascending sum of the slabs.
//
// Forward order (NOT efe_decoder's Winograd / F(2, 2) forms: the activations agree with it to rounding, not bit for bit): per output and
// per tap in (ky, kx) ascending order over the taps that reach the output, two fma chains over the input channels (16-channel chunks
// alternate between them: 32 terms each at K = 64), tap = c0 + c1, sum = sum + tap; then + bias.  Layer 4: one 32-term chain per tap.
// The data gradient uses the same scheme over the output channels.
//
// Reduction-order contract of the parameter gradient (a function of M alone, no float atomics): G = min(M, DEC_TAIL_SLABS = 32) slabs of
// P = 92 609 floats; row m belongs to slab m mod G and to row group m / DEC_TAIL_ROWS (= 64, a multiple of G: at most 2 images per slab
// and group).  Chunk, image, group and slab order: train_conv.h (layer 4's weights: 16 terms of the image per thread and tap).
// Two identical calls give identical bits.  Per-row outputs (po1, nlogpo1, d_h4, y_l) are
// computed per row with no cross-row term: they do not depend on which other rows are in the call (given the same scale).
#include "train_conv.h"

namespace efe {

using cgrad::f32x4;

// src: forward = the layer's input [rows][CI][HIN][HIN]; backward = the output gradient [rows][CO][S HIN][S HIN]
// dst: forward = relu(output) [rows][CO][S HIN][S HIN]; backward = the input gradient [rows][CI][HIN][HIN], gated by gate > 0 (same shape) if given
template <int S, int CI, int CO, int HIN, bool BWD>
__global__ void __launch_bounds__(256) k_dect_tap(const float* __restrict__ src, const float* __restrict__ W, const float* __restrict__ bias,
                                                  const float* __restrict__ gate, float* __restrict__ dst, int rows) {
#pragma clang fp contract(off)
    constexpr int OC = BWD ? CI : CO, KC = BWD ? CO : CI, HOUT = S * HIN, SD = BWD ? HOUT : HIN, NCLS = BWD ? 1 : S * S;
    constexpr int JT = HIN / 16, RG = HIN / 4, PER_ROW = (OC / 16) * NCLS * JT * RG;
    static_assert(KC % 32 == 0 && OC % 16 == 0 && HIN % 16 == 0, "whole tiles");
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW;
    int t_ = task - r * PER_ROW;
    const int rg = t_ % RG; t_ /= RG;
    const int jt = t_ % JT; t_ /= JT;
    const int cls = t_ % NCLS, oc0 = 16 * (t_ / NCLS);
    const int py = cls / S, px = cls % S;
    const int vx = 16 * jt + n, vy0 = 4 * rg;
    const float* srow = src + (size_t)r * KC * SD * SD;
    f32x4 total[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int oy, ox;              // source pixel of virtual pixel (vy, vx): (RS vy + oy, RS vx + ox)
            constexpr int RS = BWD ? S : 1;
            if (BWD) { oy = ky - 1; ox = kx - 1; }
            else {
                if (((py + 1 - ky) % S) != 0 || ((px + 1 - kx) % S) != 0) continue;       // the tap does not reach this output parity
                oy = (py + 1 - ky) / S; ox = (px + 1 - kx) / S;
            }
            const int tap = 3 * ky + kx;
            const int sx = RS * vx + ox;
            const bool okx = sx >= 0 && sx < SD;
            int soff[4]; bool ok[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sy = RS * (vy0 + t) + oy;
                ok[t] = okx && sy >= 0 && sy < SD;
                soff[t] = ok[t] ? sy * SD + sx : 0;
            }
            // A(i = n, k = q): W[ci][co][tap] with (forward) co = oc0 + n, ci = k or (backward) ci = oc0 + n, co = k
            const float* wp = BWD ? W + ((size_t)(oc0 + n) * CO) * 9 + tap : W + (size_t)(oc0 + n) * 9 + tap;
            constexpr int WK = BWD ? 9 : CO * 9;          // stride of k in W
            f32x4 c0[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
            f32x4 c1[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll 1
            for (int k0 = 0; k0 < KC; k0 += 32) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + 4 * j + q;
                    const float av = wp[(size_t)k * WK];
                    const float* sp = srow + (size_t)k * SD * SD;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        float bv = sp[soff[t]];                       // B(k = q, j = n)
                        bv = ok[t] ? bv : 0.0f;
                        if (j < 4) c0[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c0[t], 0, 0, 0);
                        else c1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, c1[t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) total[t] = total[t] + (c0[t] + c1[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int vy = vy0 + t;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int oc = oc0 + 4 * q + e;          // D(i = 4 q + e, j = n)
            float v = total[t][e];
            if (BWD) {
                const size_t idx = (((size_t)r * CI + oc) * HIN + vy) * HIN + vx;
                if (gate) v = gate_open(gate[idx]) ? v : 0.0f;
                dst[idx] = v;
            } else {
                v = relu_nan(v + bias[oc]);
                dst[(((size_t)r * CO + oc) * HOUT + (S * vy + py)) * HOUT + (S * vx + px)] = v;
            }
        }
    }
}

// layer 4 forward + sigmoid: one thread per pixel; y3 [rows][32][64][64], w4 [32][1][3][3], po [rows][4096]
__global__ void __launch_bounds__(256) k_dect_out(const float* __restrict__ y3, const float* __restrict__ w4, const float* __restrict__ b4,
                                                  float* __restrict__ po, int rows) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 4096) return;
    const int r = i >> 12, pix = i & 4095, oy = pix >> 6, ox = pix & 63;
    const float* x = y3 + (size_t)r * 32 * 4096;
    float total = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy + 1 - ky, ix = ox + 1 - kx;
            if (iy < 0 || iy > 63 || ix < 0 || ix > 63) continue;
            const float* xp = x + iy * 64 + ix;
            float c = 0.0f;
#pragma unroll 8
            for (int ci = 0; ci < 32; ++ci) c = fmaf(xp[(size_t)ci * 4096], w4[ci * 9 + 3 * ky + kx], c);
            total = total + c;
        }
    }
    const float a = total + b4[0];
    po[i] = 1.0f / (1.0f + expf(-a));
}

// one workgroup per row: nlogpo1 (k_fe_down's order) and g4 = dL / da4
__global__ void __launch_bounds__(256) k_dect_loss(const float* __restrict__ po, const float* __restrict__ o1, float scale,
                                                   float* __restrict__ nlogpo1, float* __restrict__ g4) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float D1 = 1.00001f, D0 = 0.00001f;
    const float* p = po + (size_t)r * 4096;
    const float* x = o1 + (size_t)r * 4096;
    float* g = g4 + (size_t)r * 4096;
    const float s = block_sum_of(4096, ws, [=](int i) {
#pragma clang fp contract(off)
        const float xv = x[i], pr = p[i];
        g[i] = (-scale * (xv / (D0 + pr) - (1.0f - xv) / (D1 - pr))) * ((1.0f - pr) * pr);
        return xv * logf(D0 + pr) + (1.0f - xv) * logf(D1 - pr);
    });
    if (tid == 0) nlogpo1[r] = -s;
}

// g3[ci][iy][ix] = (sum_tap g4[iy - 1 + ky][ix - 1 + kx] W4[ci][tap]) [y3 > 0]
__global__ void __launch_bounds__(256) k_dect_dx4(const float* __restrict__ g4, const float* __restrict__ w4, const float* __restrict__ y3,
                                                  float* __restrict__ g3, int rows) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * 4096) return;
    const int r = i >> 12, pix = i & 4095, iy = pix >> 6, ix = pix & 63;
    const float* g = g4 + (size_t)r * 4096;
    float gv[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int gy = iy - 1 + ky, gx = ix - 1 + kx;
            const bool ok = gy >= 0 && gy < 64 && gx >= 0 && gx < 64;
            gv[3 * ky + kx] = ok ? g[(ok ? gy : 0) * 64 + (ok ? gx : 0)] : 0.0f;
        }
#pragma unroll 4
    for (int ci = 0; ci < 32; ++ci) {
        float c = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; ++t) c = fmaf(gv[t], w4[ci * 9 + t], c);          // (an out-of-range term is an exact + 0)
        const size_t idx = ((size_t)r * 32 + ci) * 4096 + pix;
        g3[idx] = gate_open(y3[idx]) ? c : 0.0f;
    }
}

// x [rows][CI][HIN][HIN], g [rows][CO][S HIN][S HIN] -> slab[(ci CO + co) 9 + tap]; grid (CI/16 * CO/16 / 4, G)
template <int S, int CI, int CO, int HIN>
__global__ void __launch_bounds__(256) k_dect_wgrad(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ slab_w,
                                                    int rows, int P, int first) {
#pragma clang fp contract(off)
    constexpr int HOUT = S * HIN, HW = HIN * HIN;
    static_assert(HIN % 16 == 0 && HW % 32 == 0 && (CI / 16) * (CO / 16) % 4 == 0, "whole tiles");
    const int n = threadIdx.x & 15;
    const int pair = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int ci0 = 16 * (pair / (CO / 16)), co0 = 16 * (pair % (CO / 16));
    cgrad::wgrad_mfma<HW>(rows, ci0, co0, CO, slab_w + (size_t)blockIdx.y * P, first,
        [=](int r, int pos) {                                             // A(i = ci = n, k = position)
            return *reinterpret_cast<const float4*>(x + ((size_t)r * CI + ci0 + n) * HW + pos);
        },
        [=](int r, int pos, int ky, int kx) {                             // B(k = position, j = co = n)
            const int gy = S * (pos / HIN) - 1 + ky, gx = S * (pos % HIN) - 1 + kx;
            const bool ok = gy >= 0 && gy < HOUT && gx >= 0 && gx < HOUT;
            const float bv = (g + ((size_t)r * CO + co0 + n) * HOUT * HOUT)[ok ? gy * HOUT + gx : 0];
            return ok ? bv : 0.0f;
        });
}

// layer 4's weights: dW4[ci][tap] = sum y3[m][ci][iy][ix] g4[m][iy - 1 + ky][ix - 1 + kx]; grid (32, G)
__global__ void __launch_bounds__(256) k_dect_w4(const float* __restrict__ y3, const float* __restrict__ g4, float* __restrict__ slab_w,
                                                 int rows, int P, int first) {
#pragma clang fp contract(off)
    const int ci = blockIdx.x;
    cgrad::wgrad_valu(rows, 4096, slab_w + (size_t)blockIdx.y * P + ci * 9, first, [=](int r, int i, float& c, float (&t9)[9]) {
        const float* g = g4 + (size_t)r * 4096;
        const int iy = i >> 6, ix = i & 63;
        c = y3[((size_t)r * 32 + ci) * 4096 + i];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int gy = iy - 1 + ky, gx = ix - 1 + kx;
                const bool ok = gy >= 0 && gy < 64 && gx >= 0 && gx < 64;
                const float gv = g[ok ? gy * 64 + gx : 0];
                t9[3 * ky + kx] = ok ? gv : 0.0f;
            }
    });
}

// db[co] = sum_{m, positions} g[m][co][.]; grid (CO, G); slab p = slab_b + p P
__global__ void __launch_bounds__(256) k_conv_bias(const float* __restrict__ g, int CO, int HW, float* __restrict__ slab_b, int rows, int P, int first) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    const int G = gridDim.y, p = blockIdx.y, co = blockIdx.x;
    if (p >= rows) return;
    float acc_g = 0.0f;
#pragma unroll 1
    for (int r = p; r < rows; r += G) {
        const float* gp = g + ((size_t)r * CO + co) * HW;
        acc_g = acc_g + block_sum_of(HW, ws, [gp](int i) { return gp[i]; });
    }
    if (threadIdx.x == 0) cgrad::slab_put(slab_b + (size_t)p * P + co, acc_g, first);
}

void launch_conv_bias(const float* g, int CO, int HW, float* slab_b, int rows, int G, int P, int first, hipStream_t st) {
    hipLaunchKernelGGL(k_conv_bias, dim3(CO, G), dim3(256), 0, st, g, CO, HW, slab_b, rows, P, first);
}

namespace {

template <int S, int CI, int CO, int HIN, bool BWD>
void tap(const float* src, const float* W, const float* bias, const float* gate, float* dst, int rows, hipStream_t st) {
    constexpr int per_row = ((BWD ? CI : CO) / 16) * (BWD ? 1 : S * S) * (HIN / 16) * (HIN / 4);
    static_assert(per_row % 4 == 0, "whole workgroups");
    hipLaunchKernelGGL((k_dect_tap<S, CI, CO, HIN, BWD>), dim3((unsigned)((size_t)rows * per_row / 4)), dim3(256), 0, st, src, W, bias, gate, dst, rows);
}
template <int S, int CI, int CO, int HIN>
void wgrad(const float* x, const float* g, float* slab_w, int rows, int G, int first, hipStream_t st) {
    hipLaunchKernelGGL((k_dect_wgrad<S, CI, CO, HIN>), dim3((CI / 16) * (CO / 16) / 4, G), dim3(256), 0, st, x, g, slab_w, rows, DEC_TAIL_P, first);
}
void bias(const float* g, int CO, int HW, float* slab_b, int rows, int G, int first, hipStream_t st) {
    launch_conv_bias(g, CO, HW, slab_b, rows, G, DEC_TAIL_P, first, st);
}

}  // namespace

void launch_dec_tail_group(const DecTailArgs& a, hipStream_t st) {
    const int R = a.rows, G = a.G, first = a.first;
    const float* w = a.w;
    const unsigned pix_blocks = (unsigned)((size_t)R * 4096 / 256);
    // forward, activations stored
    tap<1, 64, 64, 16, false>(a.h4, w + DT_W1, w + DT_B1, nullptr, a.y1, R, st);
    tap<2, 64, 64, 16, false>(a.y1, w + DT_W2, w + DT_B2, nullptr, a.y2, R, st);
    tap<2, 64, 32, 32, false>(a.y2, w + DT_W3, w + DT_B3, nullptr, a.y3, R, st);
    hipLaunchKernelGGL(k_dect_out, dim3(pix_blocks), dim3(256), 0, st, a.y3, w + DT_W4, w + DT_B4, a.po, R);
    hipLaunchKernelGGL(k_dect_loss, dim3(R), dim3(256), 0, st, a.po, a.o1, a.scale, a.nlogpo1, a.g4);
    // layer 4
    hipLaunchKernelGGL(k_dect_w4, dim3(32, G), dim3(256), 0, st, a.y3, a.g4, a.slabs + DT_W4, R, DEC_TAIL_P, first);
    bias(a.g4, 1, 4096, a.slabs + DT_B4, R, G, first, st);
    hipLaunchKernelGGL(k_dect_dx4, dim3(pix_blocks), dim3(256), 0, st, a.g4, w + DT_W4, a.y3, a.g3, R);
    // layer 3
    wgrad<2, 64, 32, 32>(a.y2, a.g3, a.slabs + DT_W3, R, G, first, st);
    bias(a.g3, 32, 4096, a.slabs + DT_B3, R, G, first, st);
    tap<2, 64, 32, 32, true>(a.g3, w + DT_W3, nullptr, a.y2, a.g2, R, st);
    // layer 2
    wgrad<2, 64, 64, 16>(a.y1, a.g2, a.slabs + DT_W2, R, G, first, st);
    bias(a.g2, 64, 1024, a.slabs + DT_B2, R, G, first, st);
    tap<2, 64, 64, 16, true>(a.g2, w + DT_W2, nullptr, a.y1, a.g1, R, st);
    // layer 1
    wgrad<1, 64, 64, 16>(a.h4, a.g1, a.slabs + DT_W1, R, G, first, st);
    bias(a.g1, 64, 256, a.slabs + DT_B1, R, G, first, st);
    if (a.dh4) tap<1, 64, 64, 16, true>(a.g1, w + DT_W1, nullptr, nullptr, a.dh4, R, st);
}

}  // namespace efe
