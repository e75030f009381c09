// Forward free energy of one training step (/root/reference/src/torchloss.py: compute_omega, compute_loss_top, compute_loss_mid,
// compute_loss_down), the per-row tails behind the existing network runners:
//
//   k_fe_top_mid : one thread per row.  Categorical KL of the habit posterior against log_Ppi (F_top = kl_pi), omega (given per row,
//                  given as a scalar, or compute_omega(kl_pi, a, b, c, d)), and the transition KL of compute_loss_mid (F_mid).
//   k_fe_down    : one workgroup of 256 threads per row.  The Bernoulli log-likelihood of o1 under the decoder's stored image po1, summed
//                  over C*H*W in a FIXED order, the two KL vectors of compute_loss_down and the gamma-branch combination F_down.
//   k_step_omega, k_step_means : the two tails of the training step (efe_train_step): compute_omega per row between the habit net's step
//                  and the transition net's, and the eight batch statistics a training loop logs (described where they are defined).
//
// Every expression follows the reference's torch expression in the same fp32 operation order, contraction off:
//   kl(mu1, lv1, mu2, lv2, w) = 0.5 * ((lv2 - log w) - lv1) + (exp lv1 + (mu1 - mu2)^2) / ((2 exp lv2) / w) - 0.5   (torchutils.py:7-8)
//   bce(x, p)                 = x * log(1e-5 + p) + (1 - x) * log((1e-5 + 1) - p)                               (torchloss.py:62)
// kl_naive is kl with mu2 = lv2 = 0 (torch.exp(0.0) = 1 exactly).  Sums over s_dim are sequential in k.
//
// Reduction-order contract of the BCE sum (independent of launch size, chunking and image layout): the elements are indexed by their
// NCHW position i = c*H*W + p and summed by the row's workgroup in block_sum.h's order over N = C*H*W, in fp32.
// Memory-bound: per row 4 bytes of po1 and 4 of o1 per pixel (32 KiB at 1 x 64 x 64).
#include "kernels.h"
#include "block_sum.h"

namespace efe {

namespace {

__device__ __forceinline__ float kl_term(float mu1, float lv1, float mu2, float lv2, float w) {
#pragma clang fp contract(off)
    const float a = 0.5f * ((lv2 - logf(w)) - lv1);
    const float d = mu1 - mu2;
    const float num = expf(lv1) + d * d;
    const float den = (2.0f * expf(lv2)) / w;
    return (a + num / den) - 0.5f;
}

__device__ __forceinline__ float row_omega(const FeArgs& a, int r, float kl_pi) {
#pragma clang fp contract(off)
    if (a.omega_mode == 0) return a.omega_in[r];
    if (a.omega_mode == 1) return a.omega_scalar;
    // compute_omega (torchloss.py:8-9): a * (1 - 1 / (1 + exp(-(kl_pi - b) / c))) + d
    const float t = expf(-(kl_pi - a.oa_b) / a.oa_c);
    return a.oa_a * (1.0f - 1.0f / (1.0f + t)) + a.oa_d;
}

}  // namespace

// ---- the training step's two tails (efe_train_step) --------------------------------------------------------------------------------
// k_step_omega : one thread per row.  omega[r] = row_omega(a, r, kl_pi[r]): the expression k_fe_top_mid evaluates (mode 2), or the
//                caller's omega copied to the output (modes 0 / 1).  Reads a.kl_pi, writes a.omega_out; no other field of FeArgs.
__global__ void __launch_bounds__(128) k_step_omega(const FeArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.M) return;
    a.omega_out[r] = row_omega(a, r, a.omega_mode == 2 ? a.kl_pi[r] : 0.0f);
}

// k_step_means : EFE_STEP_MEANS = 8 workgroups of 256 threads, one per quantity.  Workgroup q < 7 writes means[q] = the batch mean of
//                a.x[q] [M]; workgroup 7 writes the unbiased standard deviation of a.x[1] (omega), torch.std's two passes: the mean, then
//                the sum of squared deviations from it, divided by M - 1 (0 / 0 = NaN at M = 1, as torch.std gives).
// Reduction-order contract (a function of M alone): block_sum.h's sum over the M rows in fp32, then one correctly rounded division by
// (float)M (by (float)(M - 1) for the variance) and a correctly rounded square root.  Contraction off, no atomics.  Memory-bound: 4 M
// bytes read per workgroup (8 M by the last one).
__global__ void __launch_bounds__(256) k_step_means(const StepMeansArgs a) {
#pragma clang fp contract(off)
    __shared__ float ws[4];
    const int q = blockIdx.x;
    const float* x = a.x[q < 7 ? q : 1];
    const float Mf = (float)a.M;
    const float mean = __fdiv_rn(block_sum_of(a.M, ws, [x](int r) { return x[r]; }), Mf);
    if (q < 7) {
        if (threadIdx.x == 0) a.means[q] = mean;
        return;
    }
    const float ss = block_sum_of(a.M, ws, [x, mean](int r) {
#pragma clang fp contract(off)
        const float d = x[r] - mean;
        return d * d;
    });
    if (threadIdx.x == 0) a.means[7] = __fsqrt_rn(__fdiv_rn(ss, (float)(a.M - 1)));
}

__global__ void __launch_bounds__(128) k_fe_top_mid(const FeArgs a) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.M) return;
    float kl_pi = 0.0f;
    if (a.q) {          // compute_loss_top (torchloss.py:19-26): Qpi * (log_Qpi - log_Ppi), summed over pi_dim
        for (int k = 0; k < a.A; ++k) {
            const size_t i = (size_t)r * a.A + k;
            const float t = a.q[i] * (a.logq[i] - a.log_Ppi[i]);
            if (a.kl_pi_anal) a.kl_pi_anal[i] = t;
            kl_pi = k ? kl_pi + t : t;
        }
        if (a.kl_pi) a.kl_pi[r] = kl_pi;
        if (a.F_top) a.F_top[r] = kl_pi;
    }
    const float w = row_omega(a, r, kl_pi);
    if (a.omega_out) a.omega_out[r] = w;
    if (a.q1_mean) {    // compute_loss_mid (torchloss.py:28-36): kl(qs1 | ps1) with precision omega
        float s = 0.0f;
        for (int k = 0; k < S_DIM_FE; ++k) {
            const float t = kl_term(a.q1_mean[(size_t)r * a.q1_ld + k], a.q1_lv[(size_t)r * a.q1_ld + k],
                                    a.p1_mean[(size_t)r * a.p1_ld + k], a.p1_lv[(size_t)r * a.p1_ld + k], w);
            if (a.kl_mid_anal) a.kl_mid_anal[(size_t)r * S_DIM_FE + k] = t;
            s = k ? s + t : t;
        }
        if (a.kl_mid) a.kl_mid[r] = s;
        if (a.F_mid) a.F_mid[r] = s;
    }
}

// compute_loss_down (torchloss.py:53-74) for rows [m0, m0 + gridDim.x): po is this launch's image block (row 0 = row m0)
__global__ void __launch_bounds__(256) k_fe_down(const FeArgs a, const float* po, int m0) {
#pragma clang fp contract(off)
    const int r = m0 + (int)blockIdx.x;
    __shared__ float ws[4];
    const float D1 = 1.00001f, D0 = 0.00001f;
    const int HW = a.HW, n = a.C * HW;
    const float* x = a.o1 + (size_t)r * n;
    const float* p = po + (size_t)blockIdx.x * (a.nhwc4 ? (size_t)HW * GEN_IMG_LD : (size_t)n);
    auto bce = [=](float xv, float pr) {
#pragma clang fp contract(off)
        return xv * logf(D0 + pr) + (1.0f - xv) * logf(D1 - pr);
    };
    const float logpo1 = a.nhwc4 ? block_sum_of(n, ws, [=](int i) {          // the generic path's store: pixel-major, channels padded to four
        const int c = i / HW, q = i - c * HW;
        return bce(x[i], p[(size_t)q * GEN_IMG_LD + c]);
    }) : block_sum_of(n, ws, [=](int i) { return bce(x[i], p[i]); });
    if (threadIdx.x != 0) return;
    const float w = a.omega_mode == 0 ? a.omega_in[r] : a.omega_scalar;
    float kls = 0.0f, kln = 0.0f;
    for (int k = 0; k < S_DIM_FE; ++k) {
        const float mu1 = a.q1_mean[(size_t)r * a.q1_ld + k], lv1 = a.q1_lv[(size_t)r * a.q1_ld + k];
        const float tn = kl_term(mu1, lv1, 0.0f, 0.0f, w);
        const float ts = kl_term(mu1, lv1, a.p1_mean[(size_t)r * a.p1_ld + k], a.p1_lv[(size_t)r * a.p1_ld + k], w);
        if (a.kl_naive_anal) a.kl_naive_anal[(size_t)r * S_DIM_FE + k] = tn;
        if (a.kl_s_anal) a.kl_s_anal[(size_t)r * S_DIM_FE + k] = ts;
        kln = k ? kln + tn : tn;
        kls = k ? kls + ts : ts;
    }
    // the branches compare the fp32 gamma with the fp32-rounded constants, as torch does for an fp32 0-d tensor against a Python float
    const float nb = -a.beta_o;
    float F;
    if (a.gamma <= 0.05f) F = nb * logpo1 + a.beta_s * kln;
    else if (a.gamma >= 0.95f) F = nb * logpo1 + a.beta_s * kls;
    else F = nb * logpo1 + a.beta_s * (a.gamma * kls + (1.0f - a.gamma) * kln);
    a.F_down[r] = F;
    if (a.nlogpo1) a.nlogpo1[r] = -logpo1;
    if (a.kl_s) a.kl_s[r] = kls;
    if (a.kl_naive) a.kl_naive[r] = kln;
}

void launch_step_omega(const FeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_step_omega, dim3((a.M + 127) / 128), dim3(128), 0, st, a);
}
void launch_step_means(const StepMeansArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_step_means, dim3(STEP_MEANS), dim3(256), 0, st, a);
}

void launch_fe_top_mid(const FeArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_fe_top_mid, dim3((a.M + 127) / 128), dim3(128), 0, st, a);
}
void launch_fe_down(const FeArgs& a, const float* po, int m0, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_fe_down, dim3(rows), dim3(256), 0, st, a, po, m0);
}

}  // namespace efe
