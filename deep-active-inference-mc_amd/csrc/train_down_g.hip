// The repack of ModelDown's optimiser step at every admitted geometry: every packed forward form of the generic path (generic.hip,
// generic_dec.hip, generic_enc.hip and the dense heads) rebuilt on the device from the flat master copy, behind k_adam_down (train_down.hip,
// which takes its length at run time and is reused as it is).
//
//   k_repack_down_g : k_repack_down's shape.  A gather: one thread owns one destination float4 (the fragment forms: one lane's four
//                     consecutive K elements of an MFMA fragment) or one destination float (bias tables, g_enc1p, g_wf; zero padding
//                     included), computes its source index in the master copy as the inverse of the host packer that fills the buffer at
//                     efe_commit_weights (engine_weights.hip pack_heads / pack_encoder / pack_decoder under ctx->generic) and stores.  The
//                     buffers are listed in a device-resident table of RepackDesc (build_down_repack_g, at every commit); a workgroup finds
//                     its entry by binary search over the first-block prefix.
//                     32x32x2 forms with K a multiple of 32 (g_fc4 = po_net.9.weight, rows NHWC: 7.2 M floats at 3 x 84 x 84, 16.8 M at
//                     resolution 128) take train_down.hip's 128-byte-segment thread order: thread t of a workgroup takes row t / 8 and the
//                     t % 8-th float4 of the row's 128 B, so a wave reads eight 128-B row segments and writes eight 128-B segments.
//                     The column-permuted forms of qs_net.9 (columns NHWC, col_pos = H4^2) gather scalars.
// No float atomics, no LDS, no scratch; every destination element has one owning thread.
#include "kernels.h"

namespace efe {

// (train_down.hip perm_of, restated: that kernel's listing must not change) NHWC index p * channels + c -> torch's c * positions + p
__device__ __forceinline__ int perm_of_g(int i, int channels, int positions) { return channels ? (i % channels) * positions + i / channels : i; }

__global__ void __launch_bounds__(256) k_repack_down_g(const RepackDesc* __restrict__ table, int n, const float* __restrict__ w) {
#pragma clang fp contract(off)
    int e = 0, hi = n - 1;              // the last entry whose first workgroup is not behind this one (block0 ascends strictly)
    while (e < hi) {
        const int mid = (e + hi + 1) >> 1;
        if ((int)blockIdx.x >= table[mid].block0) e = mid; else hi = mid - 1;
    }
    const RepackDesc d = table[e];
    int i = ((int)blockIdx.x - d.block0) * 256 + (int)threadIdx.x;
    if (i >= d.n) return;
    const float* src = w + d.src;
    if (d.kind == RP_BIAS) {
        d.dst[i] = i < d.out ? src[perm_of_g(i, d.row_ch, d.row_pos)] : 0.0f;
        return;
    }
    if (d.kind == RP_ENC1P) {           // g_enc1p: [tap][lane][2] <- W[co = lane % 32][ci = 2 k + lane / 32][tap], W [32][in][3][3]; zero for ci >= in
        const int k = i & 1, lane = (i >> 1) & 63, t = i >> 7;
        const int co = lane & 31, ci = 2 * k + (lane >> 5);
        d.dst[i] = ci < d.in ? src[(co * d.in + ci) * 9 + t] : 0.0f;
        return;
    }
    if (d.kind == RP_WF4) {             // g_wf: [tap][ci][c padded to 4] <- W[ci][c][tap], W [32][out][3][3]; zero for c >= out
        const int c = i & 3, ci = (i >> 2) & 31, t = i >> 7;
        d.dst[i] = c < d.out ? src[(ci * d.out + c) * 9 + t] : 0.0f;
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
        const float* row = src + (size_t)perm_of_g(co, d.row_ch, d.row_pos) * d.in;
        if (d.vec) { const float4 q = *reinterpret_cast<const float4*>(row + ci0); op[0] = q.x; op[1] = q.y; op[2] = q.z; op[3] = q.w; break; }
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = ci0 + s < d.in ? row[perm_of_g(ci0 + s, d.col_ch, d.col_pos)] : 0.0f;
        break;
    }
    case RP_DENSE16: {                  // pack_linear16: [mtile][kc][lane][4] = W[16 mt + lane % 16][16 kc + 4 (lane / 16) + s]
        const int kc = r % d.KC, mt = r / d.KC;
        const int co = mt * 16 + (lane & 15), ci0 = kc * 16 + 4 * (lane >> 4);
        if (co >= d.out) break;
        const float* row = src + (size_t)co * d.in;
        if (d.vec) { const float4 q = *reinterpret_cast<const float4*>(row + ci0); op[0] = q.x; op[1] = q.y; op[2] = q.z; op[3] = q.w; break; }
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = ci0 + s < d.in ? row[perm_of_g(ci0 + s, d.col_ch, d.col_pos)] : 0.0f;
        break;
    }
    case RP_CONV32: {                   // pack_conv, Conv2d: [tap][mtile][kc][lane][4] = W[co][ci][tap], W [out][in][3][3]
        const int kc = r % d.KC; r /= d.KC;
        const int mt = r % d.mtiles, tap = r / d.mtiles;
        const int co = mt * 32 + (lane & 31), ci0 = kc * 8 + 4 * (lane >> 5);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = (co < d.out && ci0 + s < d.in) ? src[((size_t)co * d.in + ci0 + s) * 9 + tap] : 0.0f;
        break;
    }
    default: {                          // RP_CONVT32: pack_conv, ConvTranspose2d: [tap][mtile][kc][lane][4] = W[ci][co][tap], W [in][out][3][3]
        const int kc = r % d.KC; r /= d.KC;
        const int mt = r % d.mtiles, tap = r / d.mtiles;
        const int co = mt * 32 + (lane & 31), ci0 = kc * 8 + 4 * (lane >> 5);
#pragma unroll
        for (int s = 0; s < 4; ++s) op[s] = (co < d.out && ci0 + s < d.in) ? src[((size_t)(ci0 + s) * d.out + co) * 9 + tap] : 0.0f;
        break;
    }
    }
    reinterpret_cast<float4*>(d.dst)[i] = make_float4(op[0], op[1], op[2], op[3]);
}

void launch_repack_down_g(const RepackDesc* table, int n, int blocks, const float* w, hipStream_t st) {
    hipLaunchKernelGGL(k_repack_down_g, dim3(blocks), dim3(256), 0, st, table, n, w);
}

}  // namespace efe
