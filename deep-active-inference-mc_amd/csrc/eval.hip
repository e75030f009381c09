// The epoch report (efe_eval_stats): the batch statistics the reference's train.py:136-187 appends to `stats`, reduced on the device into
// one row of EVAL_STATS floats (layout: include/efe_engine.h).  Four kernels, queued one behind the other, each field written by exactly one
// workgroup; a field whose input group is absent is written as NaN by k_eval_means.
//
//   k_eval_means  : EVAL_STATS workgroups of 256 threads, one per field.  Means, the std of kl_pi, its min / max, mse_r, and the NaN fill.
//   k_eval_median : one workgroup of 1024 threads.  The lower median of kl_pi by counting: the column is staged in LDS, every element
//                   counts the elements below it and equal to it, and the element whose rank interval holds (M - 1) / 2 is the median.
//   k_eval_tc     : one workgroup of 256 threads.  The total correlation of qs1 in fp64: column means, the 55 entries of the covariance
//                   (divisor M - 1), a Cholesky factor by one thread, (sum_k log cov_kk - 2 sum_k log L_kk) / 2, rounded once to fp32.
//   k_eval_rho    : 60 workgroups of 1024 threads, one per (latent, factor) pair.  Doubled integer ranks R = 2 #less + #equal + 1 of each
//                   column by the same O(M^2) counting sweep (one column in LDS at a time), their moments in int64, one fp64 quotient.
//
// No atomics, nothing passes between workgroups, every loop is counted by M (or Mr); LDS <= 32 KiB + 1 KiB per workgroup.
//
// Reduction-order contract of every mean, the std and mse_r (a function of the element count N alone): block_sum.h's sum in fp32, then one
// correctly rounded division by (float)N ((float)(M - 1) for the variance, then a correctly rounded square root).  Contraction off.
// k_eval_tc's fp64 sums run through the same function.
//
// Non-finite values: the sums propagate them by arithmetic.  min / max / med and the ranks are comparisons, which a NaN fails silently: each
// of them tests the bit pattern of what it stages and writes NaN when one was seen.  Integer sums and fp64 sums have no order contract to
// keep: the integer ones are exact, the fp64 ones are rounded once to fp32 at the end.
#include "kernels.h"
#include "block_sum.h"

namespace efe {

namespace {

constexpr int EV_S = 10;               // latent width (= S_DIM_FE)
constexpr int EV_WIDE = 1024;          // threads of the counting kernels
constexpr int EV_PER = EVAL_MAX_ROWS / EV_WIDE;       // elements a thread of a counting kernel owns: i = tid + k EV_WIDE, k < EV_PER

__device__ __forceinline__ bool ev_isnan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ float ev_nan() { return __uint_as_float(0x7fc00000u); }

// counts, for each of this thread's elements x[k] (k < EV_PER), the entries of col[0, M) below it and equal to it
__device__ __forceinline__ void ev_count(const float* col, int M, const float (&x)[EV_PER], int (&less)[EV_PER], int (&eq)[EV_PER]) {
#pragma unroll
    for (int k = 0; k < EV_PER; ++k) { less[k] = 0; eq[k] = 0; }
    for (int j = 0; j < M; ++j) {
        const float v = col[j];         // (one address per wave: a broadcast read)
#pragma unroll
        for (int k = 0; k < EV_PER; ++k) {
            less[k] += v < x[k] ? 1 : 0;
            eq[k] += v == x[k] ? 1 : 0;
        }
    }
}

// stages column x[r * ld] (r < M) into col, keeps this thread's elements, -> whether any thread staged a NaN (a barrier is inside)
__device__ __forceinline__ bool ev_stage(const float* x, int ld, int M, float* col, float (&mine)[EV_PER]) {
    const int tid = threadIdx.x;
    int bad = 0;
#pragma unroll
    for (int k = 0; k < EV_PER; ++k) {
        const int i = tid + k * EV_WIDE;
        mine[k] = 0.0f;
        if (i < M) {
            const float v = x[(size_t)i * ld];
            mine[k] = v; col[i] = v;
            bad |= ev_isnan(v) ? 1 : 0;
        }
    }
    return __syncthreads_or(bad) != 0;
}

}  // namespace

__global__ void __launch_bounds__(256) k_eval_means(const EvalArgs a) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    __shared__ int wi[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int M = a.M;
    const bool fe = a.row[0] != nullptr;
    float res = ev_nan();               // what an absent group leaves
    if (q == 10 || q == 12 || q >= 38) {            // med, TC, rho: their own kernels write them when the group is there
        const bool theirs = q == 10 ? fe : q == 12 ? a.qs1 != nullptr : a.s0 != nullptr;
        if (theirs) return;
    } else if (q == 13) {               // mse_r over [Mr][3 image rows][64]: the first 192 floats of every NCHW image (C = 1)
        if (a.o1_r) {
            const int N = a.Mr * 192;
            const float* o = a.o1_r; const float* p = a.po1_r;
            const float s = block_sum_of(N, ws, [o, p](int i) {
#pragma clang fp contract(off)
                const int r = i / 192, c = i - r * 192;
                const float d = o[(size_t)r * 4096 + c] - p[(size_t)r * 4096 + c];
                return d * d;
            });
            res = __fdiv_rn(s, (float)N);
        }
    } else if (fe) {
        const float Mf = (float)M;
        if (q == 0) {                   // F: (F_down + F_mid) + F_top per row (train.py:149)
            const float* ft = a.row[0]; const float* fm = a.row[1]; const float* fd = a.row[2];
            res = __fdiv_rn(block_sum_of(M, ws, [ft, fm, fd](int r) {
#pragma clang fp contract(off)
                return (fd[r] + fm[r]) + ft[r];
            }), Mf);
        } else if (q <= 7) {            // batch means; 7 = kl_pi
            const float* x = a.row[q - 1];
            res = __fdiv_rn(block_sum_of(M, ws, [x](int r) { return x[r]; }), Mf);
        } else if (q == 8 || q == 9) {  // min / max of kl_pi: an input element, or NaN when one is there
            const float* x = a.row[6];
            const bool mx = q == 9;
            float m = mx ? -INFINITY : INFINITY;
            int bad = 0;
            for (int r = tid; r < M; r += 256) {
                const float v = x[r];
                bad |= ev_isnan(v) ? 1 : 0;
                m = mx ? (v > m ? v : m) : (v < m ? v : m);
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const float o = __shfl_xor(m, off, 64);
                m = mx ? (o > m ? o : m) : (o < m ? o : m);
                bad |= __shfl_xor(bad, off, 64);
            }
            if ((tid & 63) == 0) { ws[tid >> 6] = m; wi[tid >> 6] = bad; }
            __syncthreads();
            m = ws[0];
            for (int w = 1; w < 4; ++w) m = mx ? (ws[w] > m ? ws[w] : m) : (ws[w] < m ? ws[w] : m);
            res = (wi[0] | wi[1] | wi[2] | wi[3]) ? ev_nan() : m;
        } else if (q == 11) {           // unbiased std of kl_pi: torch.std's two passes (k_step_means' omega_std)
            const float* x = a.row[6];
            const float mean = __fdiv_rn(block_sum_of(M, ws, [x](int r) { return x[r]; }), Mf);
            const float ss = block_sum_of(M, ws, [x, mean](int r) {
#pragma clang fp contract(off)
                const float d = x[r] - mean;
                return d * d;
            });
            res = __fsqrt_rn(__fdiv_rn(ss, (float)(M - 1)));
        } else {                        // 14 .. 37: column means of kl_s_anal, kl_naive_anal [M][10], kl_pi_anal [M][A]
            const float* x; int ld, k;
            if (q < 24) { x = a.kl_s_anal; ld = EV_S; k = q - 14; }
            else if (q < 34) { x = a.kl_naive_anal; ld = EV_S; k = q - 24; }
            else { x = a.kl_pi_anal; ld = a.A; k = q - 34; }
            res = __fdiv_rn(block_sum_of(M, ws, [x, ld, k](int r) { return x[(size_t)r * ld + k]; }), Mf);
        }
    }
    if (tid == 0) a.out[q] = res;
}

__global__ void __launch_bounds__(EV_WIDE) k_eval_median(const EvalArgs a) {
    __shared__ float col[EVAL_MAX_ROWS];
    __shared__ int wbest[EV_WIDE / 64];
    const int tid = threadIdx.x, M = a.M;
    float x[EV_PER];
    const bool bad = ev_stage(a.row[6], 1, M, col, x);
    int less[EV_PER], eq[EV_PER];
    ev_count(col, M, x, less, eq);
    // the element of sorted rank target: the one (any one: they are equal) whose rank interval [less, less + eq) holds it; lowest index wins
    const int target = (M - 1) / 2;
    int best = 0x7fffffff;
#pragma unroll
    for (int k = EV_PER - 1; k >= 0; --k) {
        const int i = tid + k * EV_WIDE;
        if (i < M && less[k] <= target && target < less[k] + eq[k]) best = i;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const int o = __shfl_xor(best, off, 64);
        best = o < best ? o : best;
    }
    if ((tid & 63) == 0) wbest[tid >> 6] = best;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < EV_WIDE / 64; ++w) best = wbest[w] < best ? wbest[w] : best;
    a.out[10] = (bad || best >= M) ? ev_nan() : col[best];
}

__global__ void __launch_bounds__(256) k_eval_tc(const EvalArgs a) {
#pragma clang fp contract(off)
    constexpr int NC = EV_S * (EV_S + 1) / 2;        // 55 entries of the lower triangle, (i, j <= i) at i (i + 1) / 2 + j
    __shared__ double wsum[NC][4];
    __shared__ double mean[EV_S];
    __shared__ double C[EV_S][EV_S];
    const int tid = threadIdx.x, M = a.M;
    const float* x = a.qs1;
    double acc[NC];
#pragma unroll
    for (int k = 0; k < EV_S; ++k) acc[k] = 0.0;
    for (int r = tid; r < M; r += 256) {
#pragma unroll
        for (int k = 0; k < EV_S; ++k) acc[k] = acc[k] + (double)x[(size_t)r * EV_S + k];
    }
#pragma unroll
    for (int k = 0; k < EV_S; ++k) wave_sum_put(acc[k], wsum[k]);
    __syncthreads();
    if (tid < EV_S) mean[tid] = wave_sums_join(wsum[tid]) / (double)M;
    __syncthreads();
    double mu[EV_S];
#pragma unroll
    for (int k = 0; k < EV_S; ++k) mu[k] = mean[k];
#pragma unroll
    for (int e = 0; e < NC; ++e) acc[e] = 0.0;
    for (int r = tid; r < M; r += 256) {
        double d[EV_S];
#pragma unroll
        for (int k = 0; k < EV_S; ++k) d[k] = (double)x[(size_t)r * EV_S + k] - mu[k];
#pragma unroll
        for (int i = 0; i < EV_S; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) acc[i * (i + 1) / 2 + j] = acc[i * (i + 1) / 2 + j] + d[i] * d[j];
    }
    __syncthreads();                    // (wsum is read above)
#pragma unroll
    for (int e = 0; e < NC; ++e) wave_sum_put(acc[e], wsum[e]);
    __syncthreads();
    if (tid < NC) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= tid) ++i;
        const int j = tid - i * (i + 1) / 2;
        const double c = wave_sums_join(wsum[tid]) / (double)(M - 1);
        C[i][j] = c; C[j][i] = c;
    }
    __syncthreads();
    if (tid != 0) return;
    // Cholesky, in place in the lower triangle (the diagonal of the covariance is read before it is overwritten)
    double slog_var = 0.0, slog_l = 0.0;
    bool ok = M > EV_S;                 // M <= 10 rows: a covariance of rank < 10
    for (int j = 0; j < EV_S; ++j) {
        slog_var = slog_var + log(C[j][j]);
        double p = C[j][j];
        for (int k = 0; k < j; ++k) p = p - C[j][k] * C[j][k];
        if (!(p > 0.0)) ok = false;     // (a NaN pivot too)
        const double l = sqrt(p);
        C[j][j] = l;
        slog_l = slog_l + log(l);
        for (int i = j + 1; i < EV_S; ++i) {
            double s = C[i][j];
            for (int k = 0; k < j; ++k) s = s - C[i][k] * C[j][k];
            C[i][j] = s / l;
        }
    }
    a.out[12] = ok ? (float)(0.5 * (slog_var - 2.0 * slog_l)) : ev_nan();
}

__global__ void __launch_bounds__(EV_WIDE) k_eval_rho(const EvalArgs a) {
    __shared__ float col[EVAL_MAX_ROWS];
    __shared__ long long wsum[EV_WIDE / 64][5];
    const int tid = threadIdx.x, M = a.M;
    const int li = blockIdx.x / EVAL_FACTORS, fj = blockIdx.x - li * EVAL_FACTORS;
    float x[EV_PER];
    int less[EV_PER], eq[EV_PER], rx[EV_PER];
    bool bad = ev_stage(a.s0 + li, EV_S, M, col, x);
    ev_count(col, M, x, less, eq);
#pragma unroll
    for (int k = 0; k < EV_PER; ++k) rx[k] = 2 * less[k] + eq[k] + 1;
    __syncthreads();                    // every thread is done with the first column
    bad = ev_stage(a.S_real + fj, EVAL_FACTORS, M, col, x) || bad;
    ev_count(col, M, x, less, eq);
    long long s[5] = {0, 0, 0, 0, 0};   // sum Rx, sum Ry, sum Rx^2, sum Ry^2, sum Rx Ry
#pragma unroll
    for (int k = 0; k < EV_PER; ++k) {
        if (tid + k * EV_WIDE < M) {
            const long long u = rx[k], v = 2 * less[k] + eq[k] + 1;
            s[0] += u; s[1] += v; s[2] += u * u; s[3] += v * v; s[4] += u * v;
        }
    }
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        s[e] = wave_sum(s[e]);          // (exact: integers)
        if ((tid & 63) == 0) wsum[tid >> 6][e] = s[e];
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
        s[e] = 0;
        for (int w = 0; w < EV_WIDE / 64; ++w) s[e] += wsum[w][e];
    }
    const long long n = M;
    const long long num = n * s[4] - s[0] * s[1], dx = n * s[2] - s[0] * s[0], dy = n * s[3] - s[1] * s[1];
    const double rho = (double)num / sqrt((double)dx * (double)dy);
    a.out[38 + blockIdx.x] = bad ? ev_nan() : (float)rho;
}

void launch_eval_stats(const EvalArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_means, dim3(EVAL_STATS), dim3(256), 0, st, a);
    if (a.row[0]) hipLaunchKernelGGL(k_eval_median, dim3(1), dim3(EV_WIDE), 0, st, a);
    if (a.qs1) hipLaunchKernelGGL(k_eval_tc, dim3(1), dim3(256), 0, st, a);
    if (a.s0) hipLaunchKernelGGL(k_eval_rho, dim3(EV_S * EVAL_FACTORS), dim3(EV_WIDE), 0, st, a);
}

}  // namespace efe
