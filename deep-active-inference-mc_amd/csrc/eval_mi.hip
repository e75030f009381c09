// The epoch report's second table (efe_eval_mi): the mutual information of every latent of s0 [M][10] with every true factor of
// S_real [M][6], the scores `mutual_info_regression` gives the reference's graphs/generate_traversals.py:36-46.  The estimator is
// Kraskov-Stoegbauer-Grassberger's k-nearest-neighbour one, as scikit-learn defines it for float64 columns, in fp64
// throughout with contraction off.  For one pair (latent column, factor column) and its two noise vectors:
//   1. each column: v = (double)column, sigma = sqrt(mean((v - mean v)^2)) (divisor M), sigma = 1 where sigma < 10 * 2^-52, v <- v / sigma
//   2. v <- v + ((1e-10 * max(1, mean|v|)) * noise), mean|v| of the scaled column
//   3. r_i = the k-th smallest of d_ij = max(|x_i - x_j|, |y_i - y_j|) over j != i, moved one fp64 step toward zero (zero stays zero)
//   4. nx_i = #{j != i : |x_i - x_j| <= r_i}, ny_i likewise on y
//   5. MI = max(0, psi(M) + psi(k) - mean_i psi(nx_i + 1) - mean_i psi(ny_i + 1)), rounded once to fp32
// Three kernels, queued one behind the other:
//   k_mi_cols      : 16 workgroups of 256 threads, one per column (10 latents, then 6 factors): sigma and the jitter amplitude
//                    1e-10 * max(1, mean|v / sigma|), 32 fp64 scalars.
//   k_mi_sweep<K>  : grid (ceil(M / 256), 60), 256 threads.  Workgroup (s, pair) owns the points i = 256 s + tid of its pair and sweeps all M
//                    points j past them twice, 256 at a time through LDS (thread t prepares point j0 + t of the tile): the K smallest
//                    distances by insertion into K registers, then the two marginal counts.  It writes the counts (if asked for) and the
//                    partial sums (sum psi(nx + 1), sum psi(ny + 1)) over its points.
//   k_mi_finish    : one thread per pair adds the slices' partial sums in ascending slice order and evaluates step 5.
// No atomics, nothing passes between workgroups of one kernel, every loop is counted by M; 4 KiB of LDS per workgroup of the sweep.
//
// Reduction-order contract of the three sums of steps 1 and 2 (the mean, the sum of squared deviations, the sum of |v / sigma|), a function
// of M alone: block_sum.h's sum with an fp64 accumulator, then one correctly rounded division by (double)M, a correctly rounded square
// root.  A prepared value is the same expression wherever it is formed (mi_point), so every workgroup of a pair sees the same bits.
//
// Step 5 has an order as well, because it cancels to rounding noise where the true score is 0 (four rows, or a constant column): psi comes
// from a table the context uploads once (eval_mi_psi_table: harmonic numbers by compensated summation, IEEE operations only); a slice's
// 256 values of psi(nx + 1) (0 for a thread past M) go through block_sum; the slices are added in ascending
// order from 0; MI = ((psi(M) + psi(k)) - sx / M) - sy / M, then max(0, .) and one rounding to fp32.
//
// Non-finite values: a NaN or an infinity in a column makes its sigma NaN, one in the noise makes that prepared value non-finite; every
// workgroup of a pair stages all of the pair's prepared values, tests their bit patterns and writes NaN partial sums when it saw one, so
// the pair's score is NaN and no other pair reads anything of it.
#include "kernels.h"
#include "block_sum.h"

namespace efe {

namespace {

constexpr int MI_S = 10;               // latent width
constexpr int MI_T = EVAL_MI_POINTS;   // threads = points = tile entries of a sweep workgroup
constexpr double MI_INF = __builtin_huge_val();

__device__ __forceinline__ bool mi_nonfinite(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}
__device__ __forceinline__ double mi_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// what a sweep workgroup knows of its pair: the columns, their scales and jitter amplitudes, the noise
struct MiPair {
    const float* x; const float* y;    // column bases (row strides MI_S, EVAL_FACTORS)
    double sx, sy, ax, ay;             // sigma and 1e-10 * max(1, mean|v / sigma|) of each column (k_mi_cols)
    const double* nx; const double* ny;        // injected noise [M] each, or null
    uint32_t k0, k1, stage, strx, stry;
};
// the prepared point j of the pair (steps 1 and 2)
__device__ __forceinline__ double2 mi_point(const MiPair& p, int j) {
#pragma clang fp contract(off)
    const double nx = p.nx ? p.nx[j] : (double)normal_elem(p.k0, p.k1, (uint32_t)j, p.strx, p.stage, 0, TAG_MI);
    const double ny = p.ny ? p.ny[j] : (double)normal_elem(p.k0, p.k1, (uint32_t)j, p.stry, p.stage, 0, TAG_MI);
    double2 r;
    r.x = (double)p.x[(size_t)j * MI_S] / p.sx + p.ax * nx;
    r.y = (double)p.y[(size_t)j * EVAL_FACTORS] / p.sy + p.ay * ny;
    return r;
}

}  // namespace

__global__ void __launch_bounds__(256) k_mi_cols(const EvalMiArgs a) {
#pragma clang fp contract(off)
    __shared__ double ws[4];
    const int c = blockIdx.x, M = a.M;
    const float* v = c < MI_S ? a.s0 + c : a.S_real + (c - MI_S);
    const int ld = c < MI_S ? MI_S : EVAL_FACTORS;
    const double Md = (double)M;
    const double mean = block_sum_of(M, ws, [v, ld](int i) { return (double)v[(size_t)i * ld]; }) / Md;
    const double var = block_sum_of(M, ws, [v, ld, mean](int i) {
#pragma clang fp contract(off)
        const double d = (double)v[(size_t)i * ld] - mean;
        return d * d;
    }) / Md;
    double sigma = sqrt(var);
    if (sigma < 10.0 * 2.220446049250313e-16) sigma = 1.0;      // (a NaN stays)
    const double mabs = block_sum_of(M, ws, [v, ld, sigma](int i) { return fabs((double)v[(size_t)i * ld] / sigma); }) / Md;
    if (threadIdx.x == 0) {
        a.ws[2 * c] = sigma;
        a.ws[2 * c + 1] = 1e-10 * (mabs < 1.0 ? 1.0 : mabs);    // (a NaN stays)
    }
}

template <int K>
__global__ void __launch_bounds__(MI_T) k_mi_sweep(const EvalMiArgs a) {
#pragma clang fp contract(off)
    __shared__ double2 tile[MI_T];
    __shared__ double ws[2][4];
    static_assert(MI_T == 256, "block_sum.h's workgroup");
    const int tid = threadIdx.x, M = a.M, pair = blockIdx.y, slice = blockIdx.x;
    const int li = pair / EVAL_FACTORS, fj = pair - li * EVAL_FACTORS;
    MiPair p;
    p.x = a.s0 + li; p.y = a.S_real + fj;
    p.sx = a.ws[2 * li]; p.ax = a.ws[2 * li + 1]; p.sy = a.ws[2 * (MI_S + fj)]; p.ay = a.ws[2 * (MI_S + fj) + 1];
    p.nx = a.noise ? a.noise + (size_t)(2 * pair) * M : nullptr;
    p.ny = a.noise ? a.noise + (size_t)(2 * pair + 1) * M : nullptr;
    p.k0 = a.k0; p.k1 = a.k1; p.stage = a.stage; p.strx = stream_id((uint32_t)pair, 0); p.stry = stream_id((uint32_t)pair, 1);
    const int i = slice * MI_T + tid;
    const bool live = i < M;
    double2 me; me.x = 0.0; me.y = 0.0;
    if (live) me = mi_point(p, i);
    double best[K];                     // the K smallest distances so far, ascending
#pragma unroll
    for (int q = 0; q < K; ++q) best[q] = MI_INF;
    int bad = 0;
    for (int j0 = 0; j0 < M; j0 += MI_T) {
        __syncthreads();                // every thread is done with the previous tile
        if (j0 + tid < M) {
            const double2 v = mi_point(p, j0 + tid);
            tile[tid] = v;
            bad |= (mi_nonfinite(v.x) || mi_nonfinite(v.y)) ? 1 : 0;
        }
        __syncthreads();
        const int n = M - j0 < MI_T ? M - j0 : MI_T;
        const int self = i - j0;        // the tile entry that is this thread's own point, when it is in [0, n)
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const double2 v = tile[t];  // (one address per wave: a broadcast read)
            const double dx = fabs(me.x - v.x), dy = fabs(me.y - v.y);
            double d = dx > dy ? dx : dy;
            d = t == self ? MI_INF : d;
#pragma unroll
            for (int q = 0; q < K; ++q) {       // d carries the larger one on
                const bool below = d < best[q];
                const double lo = below ? d : best[q], hi = below ? best[q] : d;
                best[q] = lo; d = hi;
            }
        }
    }
    const double kth = best[K - 1];
    const double rad = kth > 0.0 ? __longlong_as_double(__double_as_longlong(kth) - 1) : 0.0;
    int cx = 0, cy = 0;
    for (int j0 = 0; j0 < M; j0 += MI_T) {
        __syncthreads();
        if (j0 + tid < M) tile[tid] = mi_point(p, j0 + tid);
        __syncthreads();
        const int n = M - j0 < MI_T ? M - j0 : MI_T;
#pragma unroll 4
        for (int t = 0; t < n; ++t) {
            const double2 v = tile[t];
            cx += fabs(me.x - v.x) <= rad ? 1 : 0;
            cy += fabs(me.y - v.y) <= rad ? 1 : 0;
        }
    }
    cx -= 1; cy -= 1;                   // the point itself lies within any radius of itself
    if (live && a.counts) {
        a.counts[(size_t)(2 * pair) * M + i] = cx;
        a.counts[(size_t)(2 * pair + 1) * M + i] = cy;
    }
    wave_sum_put(live ? a.psi[cx + 1] : 0.0, ws[0]);       // (cx + 1 in [0, M]: entry 0, a NaN, is a poisoned point's)
    wave_sum_put(live ? a.psi[cy + 1] : 0.0, ws[1]);
    const bool anybad = __syncthreads_or(bad) != 0;        // (and block_sum's barrier between its halves, for both sums)
    if (tid != 0) return;
    double* part = a.ws + 32 + ((size_t)pair * EVAL_MI_SLICES + slice) * 2;
    part[0] = anybad ? mi_nan() : wave_sums_join(ws[0]);
    part[1] = anybad ? mi_nan() : wave_sums_join(ws[1]);
}

__global__ void __launch_bounds__(64) k_mi_finish(const EvalMiArgs a) {
#pragma clang fp contract(off)
    const int pair = threadIdx.x, M = a.M;
    if (pair >= EVAL_MI) return;
    const int slices = (M + MI_T - 1) / MI_T;
    const double* part = a.ws + 32 + (size_t)pair * EVAL_MI_SLICES * 2;
    double sx = 0.0, sy = 0.0;
    for (int s = 0; s < slices; ++s) { sx = sx + part[2 * s]; sy = sy + part[2 * s + 1]; }
    const double Md = (double)M;
    const double mi = ((a.psi[M] + a.psi[a.k]) - sx / Md) - sy / Md;
    a.out[pair] = (float)(mi < 0.0 ? 0.0 : mi);         // (a NaN stays)
}

// psi at the integers 0 .. EVAL_MI_PSI - 1 (host; the context uploads it once): psi(n) = H(n - 1) - gamma with the harmonic numbers by
// compensated (Kahan) summation in ascending order, plain IEEE operations only, so that any host and tests/eval_mi_ref.py build the same
// bits; within 4e-15 of the true values on 1 .. 8193.  Entry 0 is NaN.
void eval_mi_psi_table(double* t) {
#pragma clang fp contract(off)
    const double gamma = 0.5772156649015329;
    volatile double H = 0.0, c = 0.0;   // (volatile: the compensation must not be simplified away)
    t[0] = __builtin_nan("");
    t[1] = -gamma;
    for (int n = 1; n + 1 < EVAL_MI_PSI; ++n) {
        const double y = 1.0 / (double)n - c;
        const double s = H + y;
        c = (s - H) - y;
        H = s;
        t[n + 1] = H - gamma;
    }
}

void launch_eval_mi(const EvalMiArgs& a, hipStream_t st) {
    const dim3 grid((a.M + MI_T - 1) / MI_T, EVAL_MI);
    hipLaunchKernelGGL(k_mi_cols, dim3(MI_S + EVAL_FACTORS), dim3(256), 0, st, a);
    switch (a.k) {
        case 1: hipLaunchKernelGGL(k_mi_sweep<1>, grid, dim3(MI_T), 0, st, a); break;
        case 2: hipLaunchKernelGGL(k_mi_sweep<2>, grid, dim3(MI_T), 0, st, a); break;
        case 3: hipLaunchKernelGGL(k_mi_sweep<3>, grid, dim3(MI_T), 0, st, a); break;
        default: hipLaunchKernelGGL(k_mi_sweep<4>, grid, dim3(MI_T), 0, st, a); break;
    }
    hipLaunchKernelGGL(k_mi_finish, dim3(1), dim3(64), 0, st, a);
}

}  // namespace efe
