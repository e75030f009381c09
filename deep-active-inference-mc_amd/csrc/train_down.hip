// The optimiser step of ModelDown (encoder qs_net + decoder po_net) at 1 x 64 x 64: Adam over the flat parameter vector, then every packed
// forward form rebuilt on the device from the new raw copy.
//
//   k_adam_down   : one thread per parameter of the flat [DOWN_P] vector (parameters() order, kernels.h EQ_* / DH_* / DT_*): k_adam's
//                   arithmetic, shared with it as one inline device function (kernels.h adam_update: contraction off, division and square
//                   root correctly rounded, the bias corrections from the host in double); k_adam compiles to the instructions it had
//                   before the function was factored out.  The gradient is efe_down_grad's, already slab-summed.  Writes exp_avg,
//                   exp_avg_sq and the raw master copy only.
//   k_repack_down : a gather.  One thread owns one destination float4 (weights: one lane's four consecutive K elements of an MFMA
//                   fragment) or one destination float (bias tables, zero padding included), computes its source index in the raw copy as
//                   the inverse of the host packer that fills the buffer at efe_commit_weights (engine_weights.hip pack_heads / pack_encoder /
//                   pack_decoder) and stores.  The buffers are listed in a device-resident table of RepackDesc (built at commit); a
//                   workgroup finds its entry by the first-block prefix.  The transformed forms (Winograd F(2x2,3x3) of po_net.13, F(2,2)
//                   of po_net.15 / .17) call the host's own per-element functions (kernels.h wino_u_elem / f22_u_elem: fp64, the host's
//                   order, rounded once).
//                   32x32x2 forms with K a multiple of 32 (po_net.9.weight, 16.8 MB, nine tenths of the bytes; the other wide Linears):
//                   in fragment order the 32 lanes of a half-wave read 32 different rows, 16 B each.  So the threads of a workgroup are
//                   permuted inside their 4 KiB destination block (one 32-row tile, four K chunks): thread t takes row t / 8 and the t % 8-th
//                   float4 of the row's 128 B, so a wave reads eight 128-B row segments and writes eight 128-B segments of four fragments.
// No float atomics, no LDS, no scratch; every destination element has one owning thread.
#include "kernels.h"

namespace efe {

__global__ void __launch_bounds__(256) k_adam_down(const DownAdamArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const float g = a.g[i];
    float m = a.m[i], v = a.v[i], wv = a.w[i];
    adam_update(g, m, v, wv, a.omb1, a.b2, a.omb2, a.bc2_sqrt, a.step_size, a.eps);
    a.m[i] = m; a.v[i] = v; a.w[i] = wv;
}

// source row / column of a permuted Linear: the NHWC index p * channels + c of the kernels -> torch's channel-major c * positions + p
// (engine_weights.hip nhwc_perm)
__device__ __forceinline__ int perm_of(int i, int channels, int positions) { return channels ? (i % channels) * positions + i / channels : i; }

__global__ void __launch_bounds__(256) k_repack_down(const RepackDesc* __restrict__ table, int n, const float* __restrict__ w) {
#pragma clang fp contract(off)
    int e = 0, hi = n - 1;              // the last entry whose first workgroup is not behind this one (block0 ascends strictly): six probes of 45
    while (e < hi) {
        const int mid = (e + hi + 1) >> 1;
        if ((int)blockIdx.x >= table[mid].block0) e = mid; else hi = mid - 1;
    }
    const RepackDesc d = table[e];
    int i = ((int)blockIdx.x - d.block0) * 256 + (int)threadIdx.x;
    if (i >= d.n) return;
    const float* src = w + d.src;
    if (d.kind == RP_BIAS) {
        d.dst[i] = i < d.out ? src[perm_of(i, d.row_ch, d.row_pos)] : 0.0f;
        return;
    }
    if (d.kind == RP_TAP32) {           // [tap][32] <- [32][9]
        const int t = i >> 5, c = i & 31;
        d.dst[i] = src[c * 9 + t];
        return;
    }
    if (d.swizzle) {                    // (the file's head: a wave reads eight 128-B row segments)
        const int t = i & 255, l = t >> 3, c4 = t & 7;
        i = (i & ~255) | ((c4 >> 1) * 64 + (c4 & 1) * 32 + l);
    }
    const int lane = i & 63;
    int r = i >> 6;
    float op[4] = {0.f, 0.f, 0.f, 0.f};
    switch (d.kind) {
    case RP_DENSE32: {                  // upload_packed, one tap: [mtile][kc][lane][4] = W[32 mt + lane % 32][8 kc + 4 (lane / 32) + s]
        const int kc = r % d.KC, mt = r / d.KC;
        const int co = mt * 32 + (lane & 31), ci0 = kc * 8 + 4 * (lane >> 5);
        if (co >= d.out) break;
        const float* row = src + (size_t)perm_of(co, d.row_ch, d.row_pos) * d.in;
        if (d.vec) { const float4 q = *reinterpret_cast<const float4*>(row + ci0); op[0] = q.x; op[1] = q.y; op[2] = q.z; op[3] = q.w; break; }
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = ci0 + s < d.in ? row[perm_of(ci0 + s, d.col_ch, d.col_pos)] : 0.0f;
        break;
    }
    case RP_DENSE16: {                  // pack_linear16: [mtile][kc][lane][4] = W[16 mt + lane % 16][16 kc + 4 (lane / 16) + s]
        const int kc = r % d.KC, mt = r / d.KC;
        const int co = mt * 16 + (lane & 15), ci0 = kc * 16 + 4 * (lane >> 4);
        if (co >= d.out) break;
        const float* row = src + (size_t)co * d.in;
        if (d.vec) { const float4 q = *reinterpret_cast<const float4*>(row + ci0); op[0] = q.x; op[1] = q.y; op[2] = q.z; op[3] = q.w; break; }
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = ci0 + s < d.in ? row[perm_of(ci0 + s, d.col_ch, d.col_pos)] : 0.0f;
        break;
    }
    case RP_CONV32: {                   // pack_conv, Conv2d: [tap][mtile][kc][lane][4] = W[co][ci][tap]
        const int kc = r % d.KC; r /= d.KC;
        const int mt = r % d.mtiles, tap = r / d.mtiles;
        const int co = mt * 32 + (lane & 31), ci0 = kc * 8 + 4 * (lane >> 5);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = (co < d.out && ci0 + s < d.in) ? src[((size_t)co * d.in + ci0 + s) * 9 + tap] : 0.0f;
        break;
    }
    case RP_CONV16: {                   // the encoder's conv4: [tap][16-channel block of Cin][16-channel tile of Cout][lane][4] = W[16 mt + lane % 16][16 blk + 4 (lane / 16) + s][tap]
        const int mt = r & 3, blk = (r >> 2) & 3, tap = r >> 4;
        const int co = 16 * mt + (lane & 15), ci0 = 16 * blk + 4 * (lane >> 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = src[((size_t)co * 64 + ci0 + s) * 9 + tap];
        break;
    }
    case RP_WINO: {                     // po_net.13: the 16 Winograd matrices as taps of the 32x32x2 form, W [ci][co][3][3]
        const int kc = r % d.KC; r /= d.KC;
        const int mt = r % d.mtiles, m = r / d.mtiles;
        const int co = mt * 32 + (lane & 31), ci0 = kc * 8 + 4 * (lane >> 5);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = wino_u_elem(src + ((size_t)(ci0 + s) * d.out + co) * 9, m >> 2, m & 3);
        break;
    }
    default: {                          // RP_F22, po_net.15 / .17: pack_u16x16x4 of convt_s2_f22_weights, [U][16-channel tile][4 chunks][lane][4]
        const int kc = r & 3; r >>= 2;
        const int T = d.out / 16, ct = r % T, m = r / T;
        const int co = 16 * ct + (lane & 15), ci0 = 16 * kc + 4 * (lane >> 4);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = f22_u_elem(src + ((size_t)(ci0 + s) * d.out + co) * 9, m >> 2, m & 3);
        break;
    }
    }
    reinterpret_cast<float4*>(d.dst)[i] = make_float4(op[0], op[1], op[2], op[3]);
}

void launch_adam_down(const DownAdamArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_adam_down, dim3((a.P + 255) / 256), dim3(256), 0, st, a);
}
void launch_repack_down(const RepackDesc* table, int n, int blocks, const float* w, hipStream_t st) {
    hipLaunchKernelGGL(k_repack_down, dim3(blocks), dim3(256), 0, st, table, n, w);
}

}  // namespace efe
