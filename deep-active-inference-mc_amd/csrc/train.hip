// Training of the habit network ModelTop.qpi_net (/root/reference/src/torchmodel.py:19-25) by train_model_top
// (/root/reference/src/torchloss.py:65-74): one Adam step on F_top.mean(), F_top = sum_a Qpi (log(Qpi + 1e-20) - log_Ppi).
//
//   k_top_grad : forward + loss gradient + backward in ONE launch.  A workgroup (4 waves) takes 16-row tiles; the activations of every
//                layer stay in LDS.  Every contraction is v_mfma_f32_16x16x4_f32 (exact fp32 fma chains); the operands are gathered
//                from LDS and from the fp32 master copy of the weights (reference layout), so the transposed products of the backward
//                pass need no second packed form.
//                    forward   h_{l+1}[r][f] = act(sum_k W_l[f][k] h_l[r][k] + b_l[f])         K = layer input
//                    loss      per row: softmax, log(q + 1e-20), kl_pi, dlogit_j = (1/M) Q_j (g_j - sum_a Q_a g_a),
//                              g_a = (logQ_a - logP_a) + Q_a / (Q_a + 1e-20)                    fp32, contraction off
//                    backward  dW_l[o][i] = sum_r d_l[r][o] h_l[r][i],  db_l[o] = sum_r d_l[r][o]   K = the 16 rows of the tile
//                              d_{l-1}[r][i] = (sum_o d_l[r][o] W_l[o][i]) * [h_l[r][i] > 0]         K = layer output
//                Rows >= M of the last tile have dlogit = 0 and inputs 0: they contribute exactly zero.
//                The kernel walks a layer table (kernels.h TrainNet: widths, ReLU flag, dropout tag slot), not the habit net's sizes.
//   k_slab_sum : gradient = the fixed ascending sum of the workgroups' partial gradients (no float atomics).
//   k_adam     : one thread per parameter, torch.optim.Adam's default arithmetic; the new value goes to the fp32 master copy and to
//                both packed forward copies (32x32x2 layer-wise form, 16x16x4 fused form) through closed-form index maps.
//
// Reduction-order contract (a function of M alone): T = ceil(M / 16) tiles, G = min(T, 64) workgroups.  Workgroup p walks tiles
// p, p + G, p + 2G, ... in ascending order; a tile's contribution to an element is one MFMA chain over its rows 0..15 in ascending
// order (bias: a sequential sum), added to the workgroup's slab element by the one thread that owns it; the gradient is
// ((slab_0 + slab_1) + slab_2) + ... in ascending p.  Two identical calls give identical bits.
#include "kernels.h"

namespace efe {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 16;                          // rows per tile
constexpr int TLD = TRAIN_MAX_WIDTH + 4;        // LDS row stride in floats

__device__ __forceinline__ float slab_sum(const float* g, int nslab, int P, int i) {
#pragma clang fp contract(off)
    float s = g[i];
    for (int p = 1; p < nslab; ++p) s = s + g[(size_t)p * P + i];
    return s;
}

}  // namespace

__global__ void __launch_bounds__(256) k_top_grad(const TopGradArgs a) {
#pragma clang fp contract(off)
    __shared__ float act[TRAIN_MAX_LAYERS][TR][TLD];      // act[l] = input of layer l
    __shared__ float dl[2][TR][TLD];                      // output gradients, ping-pong (dl[0] also takes the logits)
    const TrainNet& net = *a.net;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int nl = net.nl, P = net.P, in0 = net.L[0].in;
    const int ntiles = (a.M + TR - 1) / TR;
    const float* master = net.master;
    float* slab = a.slabs + (size_t)blockIdx.x * P;
#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int r0 = tile * TR;
        const int c0 = (in0 + 15) & ~15;             // whole 16-column tiles, zero beyond the layer's width and beyond row M
        for (int i = tid; i < TR * c0; i += 256) {
            const int r = i / c0, c = i - r * c0;
            act[0][r][c] = (r0 + r < a.M && c < in0) ? a.s[(size_t)(r0 + r) * in0 + c] : 0.0f;
        }
        __syncthreads();
        // ---- forward ------------------------------------------------------------------------------------------------
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const int K = net.L[l].in, O = net.L[l].out, relu = net.L[l].relu;
            const float* W = master + net.L[l].w_off;
            const float* B = master + net.L[l].b_off;
            float (*x)[TLD] = act[l];
            float (*y)[TLD] = (l + 1 < nl) ? act[l + 1] : dl[0];
#pragma unroll 1
            for (int t = w; t < (O + 15) / 16; t += 4) {
                const int f0 = 16 * t;
                // four independent fma chains over interleaved 4-channel groups, added as ((c0 + c1) + c2) + c3: a quarter of the chain
                // length (rounding error of a long fp32 chain shows in a one-row batch) and no dependent MFMA back to back
                f32x4 acc4[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};
#pragma unroll 1
                for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int k = k0 + 4 * c + q;
                        const float av = (f0 + n < O && k < K) ? W[(size_t)(f0 + n) * K + k] : 0.0f;     // A(i = feature, k)
                        const float bv = x[n][k];                                                         // B(k, j = row); columns up to the next multiple of 16 are zero
                        acc4[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc4[c], 0, 0, 0);
                    }
                }
                const f32x4 acc = ((acc4[0] + acc4[1]) + acc4[2]) + acc4[3];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int f = f0 + 4 * q + e;
                    float v = acc[e] + B[f < O ? f : 0];
                    if (relu) v = fmaxf(v, 0.0f);
                    // (L.drop_tag != 0: the row's Philox keep mask x 2 is applied here and regenerated in the backward pass; the habit net has none)
                    y[n][f] = f < O ? v : 0.0f;
                }
            }
            __syncthreads();
        }
        // ---- loss gradient, one thread per row (torchmodel.py:27-31, torchloss.py:19-26; the 1/M of .mean() enters here) -----
        if (tid < TR) {          // (rolled loops over the A actions; Q and g of the row are parked in the free gradient buffer dl[1])
            const int row = r0 + tid, A = a.A;
            float* z = dl[0][tid];
            float* Q = dl[1][tid];
            float* g = dl[1][tid] + TRAIN_MAX_A;
            if (row < a.M) {
                float mx = z[0];
#pragma unroll 1
                for (int k = 1; k < A; ++k) mx = fmaxf(mx, z[k]);
                float sum = 0.0f;
#pragma unroll 1
                for (int k = 0; k < A; ++k) {
                    const float e = expf(z[k] - mx);
                    Q[k] = e;
                    sum = k ? sum + e : e;
                }
                float kl = 0.0f, dot = 0.0f;
#pragma unroll 1
                for (int k = 0; k < A; ++k) {
                    const float qk = Q[k] / sum;
                    const float dlg = logf(qk + 1e-20f) - a.log_Ppi[(size_t)row * A + k];
                    const float t = qk * dlg;
                    kl = k ? kl + t : t;
                    const float gk = dlg + qk / (qk + 1e-20f);
                    const float u = qk * gk;
                    dot = k ? dot + u : u;
                    Q[k] = qk; g[k] = gk;
                }
#pragma unroll 1
                for (int k = 0; k < A; ++k) z[k] = a.inv_M * (Q[k] * (g[k] - dot));
                if (a.kl_pi) a.kl_pi[row] = kl;
            } else {
#pragma unroll 1
                for (int k = 0; k < A; ++k) z[k] = 0.0f;
            }
        }
        __syncthreads();
        // ---- backward -----------------------------------------------------------------------------------------------
        int cur = 0;
#pragma unroll 1
        for (int l = nl - 1; l >= 0; --l) {
            const int K = net.L[l].in, O = net.L[l].out;
            const float* W = master + net.L[l].w_off;
            float* gW = slab + net.L[l].w_off;
            float* gB = slab + net.L[l].b_off;
            float (*d)[TLD] = dl[cur];
            float (*x)[TLD] = act[l];
            const int IT = (K + 15) / 16, OT = (O + 15) / 16;
#pragma unroll 1
            for (int t = w; t < OT * IT; t += 4) {          // dW[o][i] = sum_r d[r][o] x[r][i]
                const int ot = t / IT, o0 = 16 * ot, i0 = 16 * (t - ot * IT);
                f32x4 acc = (f32x4)(0.f);
#pragma unroll
                for (int k0 = 0; k0 < TR; k0 += 4) {
                    const float av = d[k0 + q][o0 + n];       // A(i = o, k = row)
                    const float bv = x[k0 + q][i0 + n];       // B(k = row, j = i)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = o0 + 4 * q + e, i = i0 + n;
                    if (o < O && i < K) {
                        float* p = gW + (size_t)o * K + i;
                        *p = first ? acc[e] : *p + acc[e];
                    }
                }
            }
#pragma unroll 1
            for (int o = tid; o < O; o += 256) {            // db[o] = sum_r d[r][o]
                float sm = d[0][o];
#pragma unroll
                for (int r = 1; r < TR; ++r) sm = sm + d[r][o];
                gB[o] = first ? sm : gB[o] + sm;
            }
            if (l > 0) {                                    // d_prev[r][i] = (sum_o d[r][o] W[o][i]) * [x[r][i] > 0]
                float (*dn)[TLD] = dl[cur ^ 1];
                const int relu = net.L[l - 1].relu;
#pragma unroll 1
                for (int t = w; t < IT; t += 4) {
                    const int i0 = 16 * t;
                    f32x4 acc4[4] = {(f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f), (f32x4)(0.f)};      // four chains, as in the forward pass
#pragma unroll 1
                    for (int k0 = 0; k0 < O; k0 += 16) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int o = k0 + 4 * c + q;
                            const float av = (o < O && i0 + n < K) ? W[(size_t)o * K + i0 + n] : 0.0f;  // A(i = input feature, k = o)
                            const float bv = d[n][o];                                                    // B(k = o, j = row); zero up to the next multiple of 16
                            acc4[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc4[c], 0, 0, 0);
                        }
                    }
                    const f32x4 acc = ((acc4[0] + acc4[1]) + acc4[2]) + acc4[3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int f = i0 + 4 * q + e;
                        dn[n][f] = (f < K && (!relu || x[n][f] > 0.0f)) ? acc[e] : 0.0f;
                    }
                }
                cur ^= 1;
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) k_slab_sum(const float* slabs, int nslab, int P, float* grad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) grad[i] = slab_sum(slabs, nslab, P, i);
}

// torch.optim.Adam, default flags (no amsgrad, no weight decay, not maximize), per element and in this order:
//   m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  denom = sqrt(v) / sqrt(1 - b2^t) + eps;  w = w + (-(lr / (1 - b1^t)) m) / denom
// Contraction off, division and square root correctly rounded; the bias corrections come from the host (double, rounded once).
__global__ void __launch_bounds__(256) k_adam(const AdamArgs a) {
#pragma clang fp contract(off)
    const TrainNet& net = *a.net;
    const int i = blockIdx.x * 256 + threadIdx.x, P = net.P;
    if (i >= P) return;
    const float g = slab_sum(a.g, a.nslab, P, i);
    float m = a.m[i], v = a.v[i], wv = net.master[i];
    m = m + a.omb1 * (g - m);
    v = a.b2 * v + (a.omb2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), a.bc2_sqrt) + a.eps;
    wv = wv + __fdiv_rn(-a.step_size * m, denom);        // addcdiv_(m, denom, value = -step_size): (value * m) / denom
    a.m[i] = m; a.v[i] = v; net.master[i] = wv;
    // the packed forward copies: inverses of upload_packed ([mtile 32][kc 8][lane = co % 32 + 32 (ci % 8 / 4)][ci % 4]) and
    // pack_linear16 ([mtile 16][kc 16][lane = co % 16 + 16 (ci % 16 / 4)][ci % 4]) of engine.hip
    for (int l = 0; l < net.nl; ++l) {
        const TrainLayer& L = net.L[l];
        const int e = i - L.w_off, b = i - L.b_off;
        if (e >= 0 && e < L.out * L.in) {
            const int co = e / L.in, ci = e - co * L.in;
            L.Wp32[((((size_t)(co >> 5) * L.kc32 + (ci >> 3)) * 64 + (co & 31) + 32 * ((ci >> 2) & 1)) << 2) + (ci & 3)] = wv;
            L.Wp16[((((size_t)(co >> 4) * L.kc16 + (ci >> 4)) * 64 + (co & 15) + 16 * ((ci >> 2) & 3)) << 2) + (ci & 3)] = wv;
        } else if (b >= 0 && b < L.out) {
            L.b32[b] = wv;
            L.b16[b] = wv;
        }
    }
}

void launch_top_grad(const TopGradArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_top_grad, dim3(train_slabs(a.M)), dim3(256), 0, st, a);
}
void launch_slab_sum(const float* slabs, int nslab, int P, float* grad, hipStream_t st) {
    hipLaunchKernelGGL(k_slab_sum, dim3((P + 255) / 256), dim3(256), 0, st, slabs, nslab, P, grad);
}
void launch_adam(const AdamArgs& a, int P, hipStream_t st) {
    hipLaunchKernelGGL(k_adam, dim3((P + 255) / 256), dim3(256), 0, st, a);
}

}  // namespace efe
