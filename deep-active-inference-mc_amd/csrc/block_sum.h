// The ordered sum of a 256-thread workgroup: the one reduction order of the training, loss and report kernels (loss.hip, eval.hip,
// eval_mi.hip, train_dec.hip, train_enc.hip through train_conv.h), which makes a gradient, a loss or an epoch figure a function of the
// element count alone.  tests/eval_ref.py and tests/eval_mi_ref.py replay it on the CPU; tests/test_train_bits_frozen_gpu.py holds it to the bits.
//
// Order contract, for N elements and an accumulator of type T (float, or double in the fp64 report kernels):
//   thread   : thread t of 256 adds elements t, t + 256, t + 512, ... in ascending order into an accumulator that starts at 0,
//   wave     : the 64 lanes of a wave are combined by an xor butterfly, offsets 32, 16, 8, 4, 2, 1 (acc = acc + other),
//   block    : the four wave sums are added as ((w0 + w1) + w2) + w3.
// Contraction off; no atomics; every thread of the workgroup gets the same bits.  What is summed, which N, and which division follows
// is stated where a kernel calls it.
//
// Barrier discipline: barrier, lane 0 of each wave writes ws, barrier, every thread reads ws.  The first barrier orders the write behind
// the previous call's reads, so calls may follow one another on the same ws with nothing in between; ws is block_sum's alone for as long
// as the kernel runs.  Every thread of the workgroup must reach the call.
#pragma once
#include <hip/hip_runtime.h>

namespace efe {

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma clang fp contract(off)
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// The two halves of block_sum, for a kernel that reduces several sums behind one barrier (k_eval_tc: 55 at once; k_mi_sweep: two,
// behind the __syncthreads_or it ends in; each sum with a ws[4] of its own): the wave's sum into its place of ws, and, a barrier
// later, the four of them joined.
template <class T>
__device__ __forceinline__ void wave_sum_put(T v, T* ws /*[4]*/) {
#pragma clang fp contract(off)
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
}
template <class T>
__device__ __forceinline__ T wave_sums_join(const T* ws /*[4]*/) {
#pragma clang fp contract(off)
    return ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// acc of each of the 256 threads -> the block's sum, in every thread; ws: 4 elements of LDS
template <class T>
__device__ __forceinline__ T block_sum(T acc, T* ws /*[4]*/) {
#pragma clang fp contract(off)
    __syncthreads();
    wave_sum_put(acc, ws);
    __syncthreads();
    return wave_sums_join(ws);
}

// the sum of f(i) over i < N; f may store per-element results of its own on the way
template <class T, class F>
__device__ __forceinline__ T block_sum_of(int N, T* ws /*[4]*/, F f) {
#pragma clang fp contract(off)
    T acc = (T)0;
    for (int i = threadIdx.x; i < N; i += 256) acc = acc + f(i);
    return block_sum(acc, ws);
}

}  // namespace efe
