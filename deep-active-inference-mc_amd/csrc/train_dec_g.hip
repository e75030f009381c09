// Backward of the reconstruction loss through the decoder's ConvTranspose2d tail, ModelDown.po_net[12:], at EVERY admitted geometry
// (efe_create_cfg: 1..3 colour channels, resolutions 32..128 in steps of 4): train_dec.hip's mathematics with the sizes given at run time.
//     B = the decoder's base grid (res / 4; 16 at resolution 32), C = colour channels, S3 = the third layer's stride (1 at resolution 32, else 2)
//     a1 = ConvT(64, 64, s1)(h4)   y1 = relu(a1)      [64][ B][ B]
//     a2 = ConvT(64, 64, s2)(y1)   y2 = relu(a2)      [64][2B][2B]
//     a3 = ConvT(64, 32, S3)(y2)   y3 = relu(a3)      [32][ R][ R]      R = S3 2B, the resolution
//     a4 = ConvT(32,  C, s1)(y3)   p  = sigmoid(a4)   [ C][ R][ R]
//     nlogpo1_r = -sum_{c, pixels} o log(1e-5 + p) + (1 - o) log((1e-5 + 1) - p),     L = scale * sum_r nlogpo1_r
// All NCHW; W [Cin][Cout][3][3] from a raw device copy (DT_W1 .. DT_B3 of kernels.h, then layer 4's [32][C][3][3] and [C]: DecTailGeo).
//
// Kernels (one group of at most DecTailGeo::rows_per_pass() rows per pass of launch_dec_tail_g_group); only the channel counts and the
// stride are template parameters, never a spatial size:
//   k_dectg_tap<S, CI, CO, BWD> : k_dect_tap's tap-GEMM on v_mfma_f32_16x16x4_f32 with the MFMA's column index = 16 consecutive FLATTENED
//                positions vy HIN + vx of the layer's HIN x HIN input grid (forward: the outputs (S vy + py, S vx + px) of one output
//                parity class; data gradient: the inputs).  One wave = 16 channels x four such tiles (64 consecutive positions); the
//                last wave of a class is ragged: a position >= HIN^2 feeds exact zeros, reads element 0 of its plane and stores nothing.
//                Two accumulator chains per tile and tap (16-channel chunks alternate), eight independent chains per wave.
//   k_dectg_out : layer 4 forward (VALU, one thread per (row, channel, pixel)) + sigmoid -> po1.
//   k_dectg_loss: one workgroup per row: nlogpo1 by block_sum.h's order over the C R R NCHW terms (thread t adds terms t, t + 256, ...
//                ascending, then block_sum), and g4 in k_dect_loss's expression (finite when p rounds to 0 or 1).
//   k_dectg_dx4<C> : g3 = (sum_co sum_tap g4[co][iy - 1 + ky][ix - 1 + kx] W4[ci][co][tap]) [y3 > 0]: one 9-term chain per channel, the
//                channels added in ascending order.
//   k_dectg_wgrad<S, CI, CO> : train_conv.h's wgrad_mfma_rt; a position >= HIN^2 of the ragged last chunk reads as zero in both operands.
//                A position's row and column are formed once for its nine taps, the division by a multiply-high.
//   k_dectg_w4  : layer 4's 288 C weights, one workgroup per (ci, co, slab) (wgrad_valu).
//   k_conv_bias (train_dec.hip, launch_conv_bias), k_slab_sum (train.hip).
//
// Forward and data-gradient order: train_dec.hip's (per tap in (ky, kx) ascending order two fma chains over the contracted channels,
// tap = c0 + c1, sum = sum + tap; then + bias), so at 1 x 64 x 64 the arithmetic is that of the specialised kernels.
//
// Reduction-order contract of the parameter gradient (a function of M and the geometry alone, no float atomics): G = min(M, 32) slabs of
// P floats; row m belongs to slab m mod G and to row group m / rows_per_pass().  A chunk is 32 consecutive positions of one image; chunks of
// an image, images of a group and groups of a slab are added in ascending order (train_conv.h); gradient = ((slab_0 + slab_1) + ...).
// Two identical calls give identical bits.  The per-row outputs (po1, nlogpo1, d_h4, y_l) have no cross-row term.
#include "train_conv.h"

namespace efe {

using cgrad::f32x4;

// src: forward = the layer's input [rows][CI][HIN][HIN]; backward = the output gradient [rows][CO][S HIN][S HIN]
// dst: forward = relu(output) [rows][CO][S HIN][S HIN]; backward = the input gradient [rows][CI][HIN][HIN], gated by gate > 0 (same shape) if given
template <int S, int CI, int CO, bool BWD>
__global__ void __launch_bounds__(256) k_dectg_tap(const float* __restrict__ src, const float* __restrict__ W, const float* __restrict__ bias,
                                                   const float* __restrict__ gate, float* __restrict__ dst, int rows, int HIN) {
#pragma clang fp contract(off)
    constexpr int OC = BWD ? CI : CO, KC = BWD ? CO : CI, NCLS = BWD ? 1 : S * S, RS = BWD ? S : 1;
    static_assert(KC % 32 == 0 && OC % 16 == 0, "whole channel tiles");
    const int HOUT = S * HIN, SD = BWD ? HOUT : HIN, NP = HIN * HIN, PG = (NP + 63) / 64, PER_ROW = (OC / 16) * NCLS * PG;
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (task >= rows * PER_ROW) return;
    const int r = task / PER_ROW;
    int t_ = task - r * PER_ROW;
    const int pg = t_ % PG; t_ /= PG;
    const int cls = t_ % NCLS, oc0 = 16 * (t_ / NCLS);
    const int py = cls / S, px = cls % S;
    int vy[4], vx[4]; bool okp[4];           // the lane's four virtual pixels
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int p = 64 * pg + 16 * t + n;
        okp[t] = p < NP;
        const int pc = okp[t] ? p : 0;
        vy[t] = pc / HIN; vx[t] = pc - vy[t] * HIN;
    }
    const size_t plane = (size_t)SD * SD;
    const float* srow = src + (size_t)r * KC * plane;
    f32x4 total[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int oy, ox;              // source pixel of virtual pixel (vy, vx): (RS vy + oy, RS vx + ox)
            if (BWD) { oy = ky - 1; ox = kx - 1; }
            else {
                if (((py + 1 - ky) % S) != 0 || ((px + 1 - kx) % S) != 0) continue;       // the tap does not reach this output parity
                oy = (py + 1 - ky) / S; ox = (px + 1 - kx) / S;
            }
            const int tap = 3 * ky + kx;
            int soff[4]; bool ok[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int sy = RS * vy[t] + oy, sx = RS * vx[t] + ox;
                ok[t] = okp[t] && sx >= 0 && sx < SD && sy >= 0 && sy < SD;
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
                    const float* sp = srow + (size_t)k * plane;
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
        if (!okp[t]) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int oc = oc0 + 4 * q + e;          // D(i = 4 q + e, j = n)
            float v = total[t][e];
            if (BWD) {
                const size_t idx = (((size_t)r * CI + oc) * HIN + vy[t]) * HIN + vx[t];
                if (gate) v = gate_open(gate[idx]) ? v : 0.0f;
                dst[idx] = v;
            } else {
                v = relu_nan(v + bias[oc]);
                dst[(((size_t)r * CO + oc) * HOUT + (S * vy[t] + py)) * HOUT + (S * vx[t] + px)] = v;
            }
        }
    }
}

// layer 4 forward + sigmoid: one thread per output; y3 [rows][32][R][R], w4 [32][C][3][3], po [rows][C][R][R]
__global__ void __launch_bounds__(256) k_dectg_out(const float* __restrict__ y3, const float* __restrict__ w4, const float* __restrict__ b4,
                                                   float* __restrict__ po, int rows, int C, int R) {
#pragma clang fp contract(off)
    const int RR = R * R, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * C * RR) return;
    const int r = i / (C * RR), t_ = i - r * (C * RR), co = t_ / RR, pix = t_ - co * RR, oy = pix / R, ox = pix - oy * R;
    const float* x = y3 + (size_t)r * 32 * RR;
    float total = 0.0f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy + 1 - ky, ix = ox + 1 - kx;
            if (iy < 0 || iy >= R || ix < 0 || ix >= R) continue;
            const float* xp = x + iy * R + ix;
            const float* wp = w4 + co * 9 + 3 * ky + kx;
            float c = 0.0f;
#pragma unroll 8
            for (int ci = 0; ci < 32; ++ci) c = fmaf(xp[(size_t)ci * RR], wp[ci * C * 9], c);
            total = total + c;
        }
    }
    const float a = total + b4[co];
    po[i] = 1.0f / (1.0f + expf(-a));
}

// one workgroup per row: nlogpo1 over the row's N = C R R terms and g4 = dL / da4
__global__ void __launch_bounds__(256) k_dectg_loss(const float* __restrict__ po, const float* __restrict__ o1, float scale,
                                                    float* __restrict__ nlogpo1, float* __restrict__ g4, int N) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float D1 = 1.00001f, D0 = 0.00001f;
    const float* p = po + (size_t)r * N;
    const float* x = o1 + (size_t)r * N;
    float* g = g4 + (size_t)r * N;
    const float s = block_sum_of(N, ws, [=](int i) {
#pragma clang fp contract(off)
        const float xv = x[i], pr = p[i];
        g[i] = (-scale * (xv / (D0 + pr) - (1.0f - xv) / (D1 - pr))) * ((1.0f - pr) * pr);
        return xv * logf(D0 + pr) + (1.0f - xv) * logf(D1 - pr);
    });
    if (tid == 0) nlogpo1[r] = -s;
}

// g3[ci][iy][ix] = (sum_co sum_tap g4[co][iy - 1 + ky][ix - 1 + kx] W4[ci][co][tap]) [y3 > 0]
template <int C>
__global__ void __launch_bounds__(256) k_dectg_dx4(const float* __restrict__ g4, const float* __restrict__ w4, const float* __restrict__ y3,
                                                   float* __restrict__ g3, int rows, int R) {
#pragma clang fp contract(off)
    const int RR = R * R, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * RR) return;
    const int r = i / RR, pix = i - r * RR, iy = pix / R, ix = pix - iy * R;
    const float* g = g4 + (size_t)r * C * RR;
    float gv[C][9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int gy = iy - 1 + ky, gx = ix - 1 + kx;
            const bool ok = gy >= 0 && gy < R && gx >= 0 && gx < R;
            const int off = ok ? gy * R + gx : 0;
#pragma unroll
            for (int co = 0; co < C; ++co) {
                const float v = g[co * RR + off];
                gv[co][3 * ky + kx] = ok ? v : 0.0f;
            }
        }
#pragma unroll 4
    for (int ci = 0; ci < 32; ++ci) {
        float total = 0.0f;
#pragma unroll
        for (int co = 0; co < C; ++co) {
            float c = 0.0f;
#pragma unroll
            for (int t = 0; t < 9; ++t) c = fmaf(gv[co][t], w4[(ci * C + co) * 9 + t], c);      // (an out-of-range term is an exact + 0)
            total = co == 0 ? c : total + c;
        }
        const size_t idx = ((size_t)r * 32 + ci) * RR + pix;
        g3[idx] = gate_open(y3[idx]) ? total : 0.0f;
    }
}

// x [rows][CI][HIN][HIN], g [rows][CO][S HIN][S HIN] -> slab[(ci CO + co) 9 + tap]; grid (CI/16 * CO/16 / 4, G)
// rcp = ceil(2^32 / HIN): pos / HIN = umulhi(pos, rcp), exact for every pos < 2^25 at HIN <= 128 (the error term pos (rcp HIN - 2^32)
// stays below 2^32)
struct GridPos { int iy, ix; bool in; };      // a position of the input grid: row, column, and whether it is one (< HW)
template <int S, int CI, int CO>
__global__ void __launch_bounds__(256) k_dectg_wgrad(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ slab_w,
                                                     int rows, int P, int first, int HIN, unsigned rcp) {
#pragma clang fp contract(off)
    static_assert((CI / 16) * (CO / 16) % 4 == 0, "whole workgroups");
    const int HOUT = S * HIN, HW = HIN * HIN;
    // HW a multiple of 4 (every even grid): the rows of x are 16-byte aligned and a lane's four positions lie on one side of HW, so A is one
    // 16-byte load (measured at 1 x 64 x 64, M = 50: 1.50 ms per call with this path, 1.69 ms with the four single loads alone)
    const bool quads = (HW & 3) == 0;
    const int n = threadIdx.x & 15;
    const int pair = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    const int ci0 = 16 * (pair / (CO / 16)), co0 = 16 * (pair % (CO / 16));
    // a position >= HW of the ragged last chunk: zero into both operands, the address clamped to element 0 of the plane
    cgrad::wgrad_mfma_rt(HW, rows, ci0, co0, CO, slab_w + (size_t)blockIdx.y * P, first,
        [=](int r, int pos) {                                             // A(i = ci = n, k = position)
            const float* xr = x + ((size_t)r * CI + ci0 + n) * HW;
            if (quads) {
                const bool ok = pos < HW;
                const float4 v = *reinterpret_cast<const float4*>(xr + (ok ? pos : 0));
                return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float av[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool ok = pos + s < HW;
                av[s] = xr[ok ? pos + s : 0];
                av[s] = ok ? av[s] : 0.0f;
            }
            return make_float4(av[0], av[1], av[2], av[3]);
        },
        [=](int r, GridPos at, int ky, int kx) {                          // B(k = position, j = co = n)
            const int gy = S * at.iy - 1 + ky, gx = S * at.ix - 1 + kx;
            const bool ok = at.in && gy >= 0 && gy < HOUT && gx >= 0 && gx < HOUT;
            const float bv = (g + ((size_t)r * CO + co0 + n) * HOUT * HOUT)[ok ? gy * HOUT + gx : 0];
            return ok ? bv : 0.0f;
        },
        [=](int pos) {
            GridPos at;
            at.in = pos < HW;
            const int pc = at.in ? pos : 0;
            at.iy = (int)__umulhi((unsigned)pc, rcp);
            at.ix = pc - at.iy * HIN;
            return at;
        });
}

// layer 4's weights: dW4[ci][co][tap] = sum y3[m][ci][iy][ix] g4[m][co][iy - 1 + ky][ix - 1 + kx]; grid (32 C, G), blockIdx.x = ci C + co
__global__ void __launch_bounds__(256) k_dectg_w4(const float* __restrict__ y3, const float* __restrict__ g4, float* __restrict__ slab_w,
                                                  int rows, int P, int first, int C, int R) {
#pragma clang fp contract(off)
    const int ci = blockIdx.x / C, co = blockIdx.x - ci * C, RR = R * R;
    cgrad::wgrad_valu(rows, RR, slab_w + (size_t)blockIdx.y * P + blockIdx.x * 9, first, [=](int r, int i, float& c, float (&t9)[9]) {
        const float* g = g4 + ((size_t)r * C + co) * RR;
        const int iy = i / R, ix = i - iy * R;
        c = y3[((size_t)r * 32 + ci) * RR + i];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int gy = iy - 1 + ky, gx = ix - 1 + kx;
                const bool ok = gy >= 0 && gy < R && gx >= 0 && gx < R;
                const float gv = g[ok ? gy * R + gx : 0];
                t9[3 * ky + kx] = ok ? gv : 0.0f;
            }
    });
}

namespace {

template <int S, int CI, int CO, bool BWD>
void tap(const float* src, const float* W, const float* bias, const float* gate, float* dst, int rows, int HIN, hipStream_t st) {
    const int per_row = ((BWD ? CI : CO) / 16) * (BWD ? 1 : S * S) * ((HIN * HIN + 63) / 64);
    hipLaunchKernelGGL((k_dectg_tap<S, CI, CO, BWD>), dim3((unsigned)((rows * per_row + 3) / 4)), dim3(256), 0, st, src, W, bias, gate, dst, rows, HIN);
}
template <int S, int CI, int CO>
void wgrad(const float* x, const float* g, float* slab_w, int rows, int G, int P, int first, int HIN, hipStream_t st) {
    const unsigned rcp = (unsigned)((((uint64_t)1 << 32) + (uint64_t)HIN - 1) / (uint64_t)HIN);
    hipLaunchKernelGGL((k_dectg_wgrad<S, CI, CO>), dim3((CI / 16) * (CO / 16) / 4, G), dim3(256), 0, st, x, g, slab_w, rows, P, first, HIN, rcp);
}
template <int C>
void dx4(const float* g4, const float* w4, const float* y3, float* g3, int rows, int R, hipStream_t st) {
    hipLaunchKernelGGL((k_dectg_dx4<C>), dim3((unsigned)((rows * R * R + 255) / 256)), dim3(256), 0, st, g4, w4, y3, g3, rows, R);
}

}  // namespace

void launch_dec_tail_g_group(const DecTailGArgs& a, hipStream_t st) {
    const DecTailGeo& geo = a.geo;
    const int N = a.rows, G = a.G, first = a.first, B = geo.B, C = geo.C, R = geo.R(), RR = R * R, P = geo.P();
    const bool s2 = geo.S3 == 2;
    const float* w = a.w;
    // forward, activations stored
    tap<1, 64, 64, false>(a.h4, w + DT_W1, w + DT_B1, nullptr, a.y1, N, B, st);
    tap<2, 64, 64, false>(a.y1, w + DT_W2, w + DT_B2, nullptr, a.y2, N, B, st);
    if (s2) tap<2, 64, 32, false>(a.y2, w + DT_W3, w + DT_B3, nullptr, a.y3, N, 2 * B, st);
    else tap<1, 64, 32, false>(a.y2, w + DT_W3, w + DT_B3, nullptr, a.y3, N, 2 * B, st);
    hipLaunchKernelGGL(k_dectg_out, dim3((unsigned)((N * C * RR + 255) / 256)), dim3(256), 0, st, a.y3, w + geo.w4(), w + geo.b4(), a.po, N, C, R);
    hipLaunchKernelGGL(k_dectg_loss, dim3(N), dim3(256), 0, st, a.po, a.o1, a.scale, a.nlogpo1, a.g4, C * RR);
    // layer 4
    hipLaunchKernelGGL(k_dectg_w4, dim3(32 * C, G), dim3(256), 0, st, a.y3, a.g4, a.slabs + geo.w4(), N, P, first, C, R);
    launch_conv_bias(a.g4, C, RR, a.slabs + geo.b4(), N, G, P, first, st);
    if (C == 1) dx4<1>(a.g4, w + geo.w4(), a.y3, a.g3, N, R, st);
    else if (C == 2) dx4<2>(a.g4, w + geo.w4(), a.y3, a.g3, N, R, st);
    else dx4<3>(a.g4, w + geo.w4(), a.y3, a.g3, N, R, st);
    // layer 3
    if (s2) wgrad<2, 64, 32>(a.y2, a.g3, a.slabs + DT_W3, N, G, P, first, 2 * B, st);
    else wgrad<1, 64, 32>(a.y2, a.g3, a.slabs + DT_W3, N, G, P, first, 2 * B, st);
    launch_conv_bias(a.g3, 32, RR, a.slabs + DT_B3, N, G, P, first, st);
    if (s2) tap<2, 64, 32, true>(a.g3, w + DT_W3, nullptr, a.y2, a.g2, N, 2 * B, st);
    else tap<1, 64, 32, true>(a.g3, w + DT_W3, nullptr, a.y2, a.g2, N, 2 * B, st);
    // layer 2
    wgrad<2, 64, 64>(a.y1, a.g2, a.slabs + DT_W2, N, G, P, first, B, st);
    launch_conv_bias(a.g2, 64, 4 * B * B, a.slabs + DT_B2, N, G, P, first, st);
    tap<2, 64, 64, true>(a.g2, w + DT_W2, nullptr, a.y1, a.g1, N, B, st);
    // layer 1
    wgrad<1, 64, 64>(a.h4, a.g1, a.slabs + DT_W1, N, G, P, first, B, st);
    launch_conv_bias(a.g1, 64, B * B, a.slabs + DT_B1, N, G, P, first, st);
    if (a.dh4) tap<1, 64, 64, true>(a.g1, w + DT_W1, nullptr, nullptr, a.dh4, N, B, st);
}

}  // namespace efe
