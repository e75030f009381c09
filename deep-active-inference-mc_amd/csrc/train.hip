// Training of the habit network ModelTop.qpi_net (/root/reference/src/torchmodel.py:19-25) by train_model_top
// (/root/reference/src/torchloss.py:65-74): one Adam step on F_top.mean(), F_top = sum_a Qpi (log(Qpi + 1e-20) - log_Ppi).
//
//   k_top_grad : forward + loss gradient + backward in ONE launch.  A workgroup (4 waves) takes 16-row tiles; the activations of every
//                layer stay in LDS.  The operands are gathered from LDS and from the fp32 master copy of the weights (reference layout),
//                so the transposed products of the backward pass need no second packed form.
//                    forward   h_{l+1}[r][f] = act(sum_k W_l[f][k] h_l[r][k] + b_l[f])         K = layer input
//                    loss      per row: softmax, log(q + 1e-20), kl_pi, dlogit_j = (1/M) Q_j (g_j - sum_a Q_a g_a),
//                              g_a = (logQ_a - logP_a) + Q_a / (Q_a + 1e-20)                    fp32, contraction off
//                    backward  dW_l[o][i] = sum_r d_l[r][o] h_l[r][i],  db_l[o] = sum_r d_l[r][o]   K = the 16 rows of the tile
//                              d_{l-1}[r][i] = (sum_o d_l[r][o] W_l[o][i]) * [h_l[r][i] > 0]         K = layer output
//                The kernel walks a layer table (kernels.h TrainNet: widths, ReLU flag, dropout tag slot), not the habit net's sizes.
//   k_slab_sum : gradient = the fixed ascending sum of the workgroups' partial gradients (no float atomics).
//   k_adam     : one thread per parameter, torch.optim.Adam's default arithmetic; the new value goes to the fp32 master copy and to
//                both packed forward copies (32x32x2 layer-wise form, 16x16x4 fused form) through closed-form index maps.
//
// Training of the transition network ModelMid.ps_net (torchmodel.py:41-52) by train_model_mid (torchloss.py:76-88): one Adam step on
// F_mid.mean(), F_mid = sum_k kl(q(s1) | p(s1 | s0, pi)) with precision omega (torchutils.py:7-8):
//     kl = 0.5 (lv2 - log w - lv1) + (exp(lv1) + (mu1 - mu2)^2) / den - 0.5,   den = 2 exp(lv2) / w
//     d/dmu2 = -(1/M) 2 (mu1 - mu2) / den,   d/dlv2 = (1/M) (0.5 - (exp(lv1) + (mu1 - mu2)^2) / den)          fp32, contraction off
//   k_mid_grad : the same passes for 512-wide hidden layers with MC-dropout.  k_slab_sum and k_adam serve both nets through their tables.
//
// The chain, tile, slab and gate rules are train_mlp.h's order contract.  Slabs: T = ceil(M / 16) tiles, G = min(T, 64) workgroups for
// k_top_grad, min(T, TRAIN_MID_SLABS = 8) for k_mid_grad; workgroup p owns slab p and walks tiles p, p + G, p + 2G, ... ascending.
// Both kernels keep bodies of their own, the ones they had before train_mlp.h: on its passes each measured slower than its own spread
// allows, and as written here each compiles to the listing it had.
#include "train_mlp.h"

namespace efe {

using namespace mlp;

namespace {

constexpr int TLD = TRAIN_MAX_WIDTH + 4;        // LDS row stride in floats

__device__ __forceinline__ float slab_sum(const float* g, int nslab, int P, int i) {
#pragma clang fp contract(off)
    float s = g[i];
    for (int p = 1; p < nslab; ++p) s = s + g[(size_t)p * P + i];
    return s;
}

}  // namespace

// k_top_grad: act[l] plus a ping-pong dl in LDS; dW tiles dealt to the four waves one by one (on train_mlp.h's dw_pass, where a wave owns 16
// outputs, it was 5 % slower at M = 4096).  Per element its dW / db chains are train_mlp.h's tile rule.
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
                    if (relu) v = relu_nan(v);
                    // (the habit net has no dropout: L.drop_tag is 0 in its table; k_mid_grad below is the kernel for layers that carry one)
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
                        dn[n][f] = (f < K && (!relu || gate_open(x[n][f]))) ? acc[e] : 0.0f;
                    }
                }
                cur ^= 1;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// k_mid_grad: the same three passes for the transition net ModelMid.ps_net (torchmodel.py:41-52): Linear(A + 10, 512), three times
// ReLU + Dropout(0.5) with 512-wide Linears between, Linear(512, 20) = ps1_mean | ps1_logvar; loss = mean_r sum_k kl (header).
//
// LDS (dynamic, MID_LDS_BYTES = 102 656): X0 [16][20] the input tile | H1, H2, H3 [16][516] the post-mask activations (H_l = input of
// layer l) | DO [16][36] the output tile (logits, then their gradient).  d_l sits in H_{l+1} (DO for the last layer).  One workgroup per CU.
//
// Dropout: the forward pass draws the keep mask of hidden layer li as k_trans_fused does (tag TAG_MID + li = TrainLayer::drop_tag, block
// f >> 7, the call's row / stream / stage) and stores relu(a) * mask (kept value x 2).
//
// Chains: train_mlp.h's chain rule with SIXTEEN accumulators (32 terms per accumulator at K = 512), joined by tree16() = tree<16> of that
// header, written out here (with the header's tree<16>, mask_block or contract in its place the kernel compiles to another listing, and
// on contract / dprev_pass it measured 7.130 -> 7.165 ms at M = 1024 against a spread of 0.010 ms).  The forward pass reads the packed 16x16x4 copy
// (one coalesced float4 per lane and chunk), the transposed product gathers W[o][i] from the master copy; dW is one 16-term chain per tile.  The forward order is not
// k_trans_fused's single chain: ps1_mean / ps1_logvar agree with efe_loss_mid to rounding, not bit for bit.
namespace {

constexpr int MLD = TRAIN_MID_WIDTH + 4;          // row stride of H1..H3 (516 floats: rows 16-byte aligned, 16 rows on 64 distinct banks)
constexpr int XLD = TRAIN_MID_IN + 4;             // ... of X0
constexpr int OLD = TRAIN_MID_OUT + 4;            // ... of DO
constexpr int MID_LDS_BYTES = (TR * XLD + 3 * TR * MLD + TR * OLD) * (int)sizeof(float);

__device__ __forceinline__ f32x4 tree16(const f32x4 (&a)[16]) {
#pragma clang fp contract(off)
    const f32x4 b0 = (a[0] + a[1]) + (a[2] + a[3]), b1 = (a[4] + a[5]) + (a[6] + a[7]);
    const f32x4 b2 = (a[8] + a[9]) + (a[10] + a[11]), b3 = (a[12] + a[13]) + (a[14] + a[15]);
    return (b0 + b1) + (b2 + b3);
}

}  // namespace

__global__ void __launch_bounds__(256, 1) k_mid_grad(const MidGradArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float mid_sm[];
    const TrainNet& net = *a.net;
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, q = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nl = net.nl, P = net.P, in0 = net.L[0].in, S = a.S;
    const int ntiles = (a.M + TR - 1) / TR;
    const float* master = net.master;
    float* slab = a.slabs + (size_t)blockIdx.x * P;
    float* const X0 = mid_sm;
    float* const H = mid_sm + TR * XLD;              // H + (l - 1) * TR * MLD = input of layer l >= 1
    float* const DO = H + 3 * TR * MLD;
    // input / output buffer of layer l and their row strides
    auto xin = [&](int l) { return l == 0 ? X0 : H + (l - 1) * TR * MLD; };
    auto xld = [&](int l) { return l == 0 ? XLD : MLD; };
    auto yout = [&](int l) { return l + 1 < nl ? H + l * TR * MLD : DO; };
    auto yld = [&](int l) { return l + 1 < nl ? MLD : OLD; };
#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const bool first = tile == (int)blockIdx.x;
        const int r0 = tile * TR;
        for (int i = tid; i < TR * TRAIN_MID_IN; i += 256) {         // [pi0 | s0], zero beyond the layer's width and beyond row M
            const int r = i / TRAIN_MID_IN, c = i - r * TRAIN_MID_IN, row = r0 + r;
            float v = 0.0f;
            if (row < a.M && c < in0) v = c < a.A ? a.pi0[(size_t)row * a.A + c] : a.s0[(size_t)row * S + (c - a.A)];
            X0[r * XLD + c] = v;
        }
        __syncthreads();
        // ---- forward ------------------------------------------------------------------------------------------------
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const TrainLayer& L = net.L[l];
            const int O = L.out, KC = L.kc16, relu = L.relu, OT = (O + 15) / 16, tpw = (OT + 3) / 4;
            const uint32_t tag = (uint32_t)L.drop_tag;
            const float* B = master + L.b_off;
            const float* x = xin(l) + n * xld(l) + 4 * q;
            float* y = yout(l) + n * yld(l);
            const int t1 = min(OT, (w + 1) * tpw);
#pragma unroll 1
            for (int t = w * tpw; t < t1; ++t) {                  // a wave's tiles are contiguous: 8 tiles = one Philox block at O = 512
                const int f0 = 16 * t;
                const float4* Wp = reinterpret_cast<const float4*>(L.Wp16) + (size_t)t * KC * 64 + lane;
                f32x4 acc[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) acc[j] = (f32x4)(0.f);
#pragma unroll 1
                for (int c0 = 0; c0 < KC; c0 += 16) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int c = c0 + j;
                        if (c < KC) {
                            const float4 av = Wp[(size_t)c * 64];                                     // A(i = feature, k): W[f0 + n][16 c + 4 q + s]
                            const float4 bv = *reinterpret_cast<const float4*>(x + 16 * c);            // B(k, j = row):     x[n][16 c + 4 q + s]
                            mfma4(acc[j], av.x, av.y, av.z, av.w, bv);
                        }
                    }
                }
                const f32x4 sum = tree16(acc);
                uint32_t word = 0xFFFFFFFFu;
                if (tag) {
                    uint32_t k0 = a.key.k0, k1 = a.key.k1;
                    asm volatile("" : "+v"(k0), "+v"(k1));
                    const uint4 rnd = noise_words(k0, k1, tag, (uint32_t)(f0 >> 7), a.key.row0 + (uint32_t)(r0 + n), a.key.stream, a.key.stage);
                    const int wsel = (f0 >> 5) & 3;
                    word = wsel == 0 ? rnd.x : wsel == 1 ? rnd.y : wsel == 2 ? rnd.z : rnd.w;
                }
                float4 out;
                float* o4 = &out.x;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int f = f0 + 4 * q + e;
                    float v = sum[e] + B[f < O ? f : 0];
                    if (relu) v = relu_nan(v);
                    if (tag) v = v * keep2(((word >> (f & 31)) & 1u));
                    o4[e] = f < O ? v : 0.0f;
                }
                *reinterpret_cast<float4*>(y + f0 + 4 * q) = out;
            }
            __syncthreads();
        }
        // ---- loss gradient, one thread per row (torchloss.py:28-37, torchutils.py:7-8; the 1/M of .mean() enters here) -------------
        if (tid < TR) {
            const int row = r0 + tid;
            float* z = DO + tid * OLD;                  // mean 0..S-1 | logvar S..2S-1, replaced by their gradients
            if (row < a.M) {
                const float om = a.omega_mode == 0 ? a.omega_in[row] : a.omega_scalar;
                const float log_om = logf(om);
                float F = 0.0f;
#pragma unroll 1
                for (int k = 0; k < S; ++k) {
                    const float mu1 = a.q1_mean[(size_t)row * S + k], lv1 = a.q1_lv[(size_t)row * S + k], mu2 = z[k], lv2 = z[S + k];
                    a.p1_mean[(size_t)row * S + k] = mu2;
                    a.p1_lv[(size_t)row * S + k] = lv2;
                    const float h = 0.5f * ((lv2 - log_om) - lv1);        // kl_term of loss.hip, operation for operation
                    const float d = mu1 - mu2;
                    const float num = expf(lv1) + d * d;
                    const float den = (2.0f * expf(lv2)) / om;
                    const float ratio = num / den;
                    const float t = (h + ratio) - 0.5f;
                    F = k ? F + t : t;
                    z[k] = a.inv_M * (-((2.0f * d) / den));
                    z[S + k] = a.inv_M * (0.5f - ratio);
                }
                a.F_mid[row] = F;
            } else {
#pragma unroll 1
                for (int k = 0; k < 2 * S; ++k) z[k] = 0.0f;
            }
        }
        __syncthreads();
        // ---- backward -----------------------------------------------------------------------------------------------
#pragma unroll 1
        for (int l = nl - 1; l >= 0; --l) {
            const TrainLayer& L = net.L[l];
            const int K = L.in, O = L.out;
            const float* W = master + L.w_off;
            float* gW = slab + L.w_off;
            float* gB = slab + L.b_off;
            const float* d = yout(l);                  // d_l lives where layer l's output was
            const int dld = yld(l);
            float* x = xin(l);
            const int xs = xld(l);
            const int IT = (K + 15) / 16, OT = (O + 15) / 16;
#pragma unroll 1
            for (int ot = w; ot < OT; ot += 4) {                  // dW[o][i] = sum_r d[r][o] x[r][i]: A(i = o, k = row) stays in registers over the i tiles
                const int o0 = 16 * ot;
                float av[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) av[c] = d[(4 * c + q) * dld + o0 + n];
#pragma unroll 2
                for (int it = 0; it < IT; ++it) {
                    const int i0 = 16 * it;
                    f32x4 acc = (f32x4)(0.f);
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], x[(4 * c + q) * xs + i0 + n], acc, 0, 0, 0);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int o = o0 + 4 * q + e, i = i0 + n;
                        if (o < O && i < K) {
                            float* p = gW + (size_t)o * K + i;
                            *p = first ? acc[e] : *p + acc[e];
                        }
                    }
                }
            }
#pragma unroll 1
            for (int o = tid; o < O; o += 256) {                  // db[o] = sum_r d[r][o]
                float sm = d[o];
#pragma unroll
                for (int r = 1; r < TR; ++r) sm = sm + d[r * dld + o];
                gB[o] = first ? sm : gB[o] + sm;
            }
            __syncthreads();                                      // dW_l has consumed x = H_l: it may now be overwritten
            if (l > 0) {                                          // d_{l-1}[r][i] = (sum_o d[r][o] W[o][i]) * mask[r][i] [a[r][i] > 0], written over H_l[r][i]
                const TrainLayer& Lp = net.L[l - 1];
                const float keep = Lp.drop_tag ? 2.0f : 1.0f;
                const int OC = OT, tpw = (IT + 3) / 4, t1 = min(IT, (w + 1) * tpw);
                const float* dn = d + n * dld + 4 * q;
#pragma unroll 1
                for (int t = w * tpw; t < t1; ++t) {
                    const int i0 = 16 * t;
                    const float* Wc = W + i0 + n;              // (K = the width of a hidden layer: whole 16-feature tiles)
                    f32x4 acc[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) acc[j] = (f32x4)(0.f);
#pragma unroll 1
                    for (int c0 = 0; c0 < OC; c0 += 16) {
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const int c = c0 + j;
                            if (c < OC) {
                                const int o = 16 * c + 4 * q;
                                const float4 bv = *reinterpret_cast<const float4*>(dn + 16 * c);       // B(k = o, j = row): d[n][16 c + 4 q + s]
                                float av[4];                                                           // A(i = input feature, k = o): W[o][i0 + n]; beyond O the
#pragma unroll                                                                                                 // row index is clamped: d is zero there, the product exactly 0
                                for (int s = 0; s < 4; ++s) av[s] = Wc[(size_t)min(o + s, O - 1) * K];
                                mfma4(acc[j], av[0], av[1], av[2], av[3], bv);
                            }
                        }
                    }
                    const f32x4 sum = tree16(acc);
                    float* hp = x + n * xs + i0 + 4 * q;
                    const float4 h = *reinterpret_cast<const float4*>(hp);
                    float4 g;
                    g.x = gated(h.x, keep * sum[0], Lp.relu, keep != 1.0f);
                    g.y = gated(h.y, keep * sum[1], Lp.relu, keep != 1.0f);
                    g.z = gated(h.z, keep * sum[2], Lp.relu, keep != 1.0f);
                    g.w = gated(h.w, keep * sum[3], Lp.relu, keep != 1.0f);
                    *reinterpret_cast<float4*>(hp) = g;
                }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(256) k_slab_sum(const float* slabs, int nslab, int P, float* grad) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) grad[i] = slab_sum(slabs, nslab, P, i);
}

// torch.optim.Adam, default flags (no amsgrad, no weight decay, not maximize), per element: kernels.h adam_update (shared with
// train_down.hip's k_adam_down), then the element's two packed forward copies.
__global__ void __launch_bounds__(256) k_adam(const AdamArgs a) {
#pragma clang fp contract(off)
    const TrainNet& net = *a.net;
    const int i = blockIdx.x * 256 + threadIdx.x, P = net.P;
    if (i >= P) return;
    const float g = slab_sum(a.g, a.nslab, P, i);
    float m = a.m[i], v = a.v[i], wv = net.master[i];
    adam_update(g, m, v, wv, a.omb1, a.b2, a.omb2, a.bc2_sqrt, a.step_size, a.eps);
    a.m[i] = m; a.v[i] = v; net.master[i] = wv;
    // the packed forward copies: inverses of upload_packed ([mtile 32][kc 8][lane = co % 32 + 32 (ci % 8 / 4)][ci % 4]) and
    // pack_linear16 ([mtile 16][kc 16][lane = co % 16 + 16 (ci % 16 / 4)][ci % 4]) of engine_weights.hip
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
void launch_mid_grad(const MidGradArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_mid_grad, dim3(train_mid_slabs(a.M)), dim3(256), MID_LDS_BYTES, st, a);
}
int init_train_kernels() {
    return hipFuncSetAttribute((const void*)k_mid_grad, hipFuncAttributeMaxDynamicSharedMemorySize, MID_LDS_BYTES) != hipSuccess;
}
void launch_slab_sum(const float* slabs, int nslab, int P, float* grad, hipStream_t st) {
    hipLaunchKernelGGL(k_slab_sum, dim3((P + 255) / 256), dim3(256), 0, st, slabs, nslab, P, grad);
}
void launch_adam(const AdamArgs& a, int P, hipStream_t st) {
    hipLaunchKernelGGL(k_adam, dim3((P + 255) / 256), dim3(256), 0, st, a);
}

}  // namespace efe
