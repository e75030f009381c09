// The parameter-gradient passes of the 3 x 3 convolutions: the decoder's ConvTranspose2d tail (train_dec.hip) and the encoder's Conv2d
// stack (train_enc.hip) build k_dect_wgrad / k_enc_wgrad, k_dect_w4 / k_enc_w1 and the one bias kernel of them.  A kernel decodes its
// indices, says how an operand is fetched, and makes one call.
//
// Order contract of a weight or bias gradient (a function of M alone, no float atomics; every (element, slab) has ONE owning thread):
// workgroup (., p) of a grid (., G) owns slab p and walks the rows r = p, p + G, ... of its row group.  Per element and slab:
//   chunk  : one chain of 8 v_mfma_f32_16x16x4_f32 over 32 consecutive positions of one image: half h = 0, 1, step s = 0..3 contracts
//            positions pos0 + 16 h + 4 q + s of the four lane groups q.  (The VALU weights: per thread the positions t, t + 256, ...
//            ascending on one fma chain per tap; the biases: the plain sum; then block_sum.h's ordered sum.)
//   image  : the chunks of an image added in ascending order,
//   group  : the images of the slab inside one row group added in ascending order,
//   slab   : the row groups added in ascending order (slab_put: first ? v : *d + v);   gradient = ((slab_0 + slab_1) + slab_2) + ...
//            (k_slab_sum, train.hip).
// Lane (n, q) = (lane & 15, lane >> 4) feeds A(i = n, k = q) and B(k = q, j = n) and holds D(i = 4 q + e, j = n).  A carries the channel
// that is W's first index, B the one that is its second: W is [Cin][Cout][3][3] for ConvTranspose2d, [Cout][Cin][3][3] for Conv2d.
//
// Deliberately NOT here: the forward and data-gradient kernels (k_dect_tap<.., BWD>, k_enc_conv, k_enc_dx, k_enc_conv1, k_dect_out,
// k_dect_dx4).  Their chains differ in structure (two alternating chains per tap, three per kernel row, one per tap; 4 x 16 virtual
// pixels against 16 flattened positions), the stored bits pin each of them, and one body would take a flag per difference.  Nor the host
// side (engine_train.hip's DecGrad / EncGrad), nor anything on the rollout path.
#pragma once
#include "kernels.h"
#include "block_sum.h"

namespace efe {
namespace cgrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void slab_put(float* d, float v, int first) {
#pragma clang fp contract(off)
    *d = first ? v : *d + v;
}

// dW of one 16 x 16 channel tile (origins i0, j0 of W's first and second index, NJ = the extent of the second) for all nine taps, over
// images of HW positions; slab = this workgroup's.  lda(r, pos) -> the lane's A values of positions pos .. pos + 3 of row r;
// ldb(r, where(pos), ky, kx) -> its B value of position pos under tap (ky, kx).  A position >= HW of a ragged last chunk must give zero in both.
// The call is the kernel's last statement.  HW is a run-time value here (train_dec_g.hip: the geometry is the context's); wgrad_mfma<HW>
// below is the same body with the extent known to the compiler.  where(pos) -> what ldb takes in place of the position, formed ONCE per
// position for its nine taps (run-time extents: the position's row and column, which cost a division).
template <class LA, class LB, class LW>
__device__ __forceinline__ void wgrad_mfma_rt(int HW, int rows, int i0, int j0, int NJ, float* slab, int first, LA lda, LB ldb, LW where) {
#pragma clang fp contract(off)
    const int G = gridDim.y, p = blockIdx.y;
    if (p >= rows) return;
    const int lane = threadIdx.x & 63, n = lane & 15, q = lane >> 4;
    f32x4 acc_g[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc_g[t] = (f32x4)(0.f);
#pragma unroll 1
    for (int r = p; r < rows; r += G) {
        f32x4 acc_i[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc_i[t] = (f32x4)(0.f);
#pragma unroll 1
        for (int pos0 = 0; pos0 < HW; pos0 += 32) {
            f32x4 ch[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) ch[t] = (f32x4)(0.f);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pos = pos0 + 16 * h + 4 * q;
                const float4 a4 = lda(r, pos);
                const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const auto at = where(pos + s);
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
                            ch[3 * ky + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], ldb(r, at, ky, kx), ch[3 * ky + kx], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t) acc_i[t] = acc_i[t] + ch[t];
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) acc_g[t] = acc_g[t] + acc_i[t];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) slab_put(slab + ((size_t)(i0 + 4 * q + e) * NJ + j0 + n) * 9 + t, acc_g[t][e], first);
}

template <int HW, class LA, class LB>
__device__ __forceinline__ void wgrad_mfma(int rows, int i0, int j0, int NJ, float* slab, int first, LA lda, LB ldb) {
    wgrad_mfma_rt(HW, rows, i0, j0, NJ, slab, first, lda, ldb, [](int pos) { return pos; });
}

// the nine weights of one channel pair on the VALU (a layer with one channel on one side): slab9 = their place in this workgroup's
// slab.  fetch(r, i, c, t9): the centre value c of position i < N of row r and its nine tap partners (zero where a tap falls outside).
// Thread t < 9 owns tap t.  The call is the kernel's last statement.
template <class F>
__device__ __forceinline__ void wgrad_valu(int rows, int N, float* slab9, int first, F fetch) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    const int G = gridDim.y, p = blockIdx.y, tid = threadIdx.x;
    if (p >= rows) return;
    float acc_g = 0.0f;
#pragma unroll 1
    for (int r = p; r < rows; r += G) {
        float a9[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) a9[t] = 0.0f;
#pragma unroll 1
        for (int i = tid; i < N; i += 256) {
            float c, t9[9];
            fetch(r, i, c, t9);
#pragma unroll
            for (int t = 0; t < 9; ++t) a9[t] = fmaf(c, t9[t], a9[t]);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float s = block_sum(a9[t], ws);
            if (tid == t) acc_g = acc_g + s;
        }
    }
    if (tid < 9) slab_put(slab9 + tid, acc_g, first);
}

}  // namespace cgrad

// db[co] = sum_{m, positions} g[m][co][.] of a layer with CO channels of HW positions, into element co of each of the G slabs of P floats
// at slab_b: k_conv_bias, grid (CO, G).  ONE kernel for both files; train_dec.hip defines it and this launcher.
void launch_conv_bias(const float* g, int CO, int HW, float* slab_b, int rows, int G, int P, int first, hipStream_t st);

}  // namespace efe
