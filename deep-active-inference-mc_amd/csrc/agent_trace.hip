// The record of an agent run (what the reference's test_demo.py shows on every tick) kept in device arrays, T rows (ticks) x E games:
//
//   k_agent_trace_tick    : the environment as the tick's decision sees it, the action the tick's act will execute and the queue length
//   k_agent_trace_decision: what the deciding games decided -- choice, uniform, G and the three terms (test_demo.py:152-155), the
//                           distribution the action was drawn from (agent_probs, the function k_agent_choose draws from) and the planned path
//   k_agent_plan_mask     : make_mask (test_demo.py:87-113) over the planner's history of one decision
//   k_agent_view          : the frame the demo draws (test_demo.py:206-215) as uint8, saturating
//
// The record is allocated pre-filled with "nothing happened" values, so no kernel initialises a row: each writes only what happened.
// Nothing here writes an array of efe_agent or of the environment, so a recorded run and an unrecorded one take the same trajectory.
#include "kernels.h"

namespace efe {

// One thread = one game.  Launched after the tick's decision and before its act: the head of the queue is the action act executes.
__global__ void __launch_bounds__(128) k_agent_trace_tick(const AgentState a, const AgentTrace tr, int row, const float* state, const float* last_r) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= tr.E) return;
    const size_t o = (size_t)row * tr.E + e;
    for (int k = 0; k < 7; ++k) tr.state[o * 7 + k] = state[(size_t)e * 7 + k];
    tr.last_r[o] = last_r[e];
    const int len = a.len[e], head = a.head[e];
    const bool queued = len >= 1 && head >= 0 && head + len <= a.cap;        // k_agent_act's test: such a game moves
    tr.action[o] = queued ? a.queue[(size_t)e * a.cap + head] : -1;
    tr.queue_len[o] = len;
}
void launch_agent_trace_tick(const AgentState& a, const AgentTrace& tr, int row, const float* state, const float* last_r, hipStream_t st) {
    hipLaunchKernelGGL(k_agent_trace_tick, dim3((tr.E + 127) / 128), dim3(128), 0, st, a, tr, row, state, last_r);
}

// Deciding game i (of n) is game ids[i]; its entries of row `row` are written, those of the other games keep their fill values.
//   mode AGENT_AI / T1 / T12: G = sum_G / steps, terms = (-sum_terms[0] / steps, sum_terms[1] / steps, sum_terms[2] / steps), one fp32
//                             division each, and probs = agent_probs for the mode
//   mode AGENT_PROBS        : probs = probs [n][4] (the habit posterior)
//   mode AGENT_NONE         : no distribution
// choice, u, path / path_len (all NULL ok) are copied where given; a slot with path_len[i] < 0 queued no planned path and keeps the fill.
__global__ void __launch_bounds__(128) k_agent_trace_decision(const AgentTrace tr, int row, const int32_t* ids, int n, int mode, const int32_t* choice,
                                                              const float* u, const float* sum_G, const float* sum_terms, const float* probs,
                                                              int steps, float temperature, const int32_t* path, const int32_t* path_len,
                                                              int path_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = ids[i];
    if (g < 0 || g >= tr.E) return;                                  // memory safety only: efe_agent_need writes ids in range
    const size_t o = (size_t)row * tr.E + g;
    tr.decided[o] = 1;
    if (choice) tr.choice[o] = choice[i];
    if (u) tr.u[o] = u[i];
    if (mode != AGENT_NONE) {
        float p[4];
        agent_probs(mode, i, n, sum_G, sum_terms, probs, steps, temperature, p);
        for (int k = 0; k < 4; ++k) tr.probs[o * 4 + k] = p[k];
    }
    if (mode == AGENT_AI || mode == AGENT_T1 || mode == AGENT_T12) {
        const float fs = (float)steps;
        for (int k = 0; k < 4; ++k) {
            const size_t r = (size_t)i * 4 + k;
            tr.G[o * 4 + k] = sum_G[r] / fs;
            tr.terms[o * 12 + k] = -sum_terms[r] / fs;
            tr.terms[o * 12 + 4 + k] = sum_terms[(size_t)n * 4 + r] / fs;
            tr.terms[o * 12 + 8 + k] = sum_terms[(size_t)n * 8 + r] / fs;
        }
    }
    if (path && path_len && path_len[i] >= 0) {
        const int len = path_len[i];
        tr.path_len[o] = len;                                        // the true length, also above Lp
        for (int k = 0; k < len && k < tr.Lp && k < path_stride; ++k) tr.path[o * tr.Lp + k] = path[(size_t)i * path_stride + k];
    }
}
void launch_agent_trace_decision(const AgentTrace& tr, int row, const int32_t* ids, int n, int mode, const int32_t* choice, const float* u,
                                 const float* sum_G, const float* sum_terms, const float* probs, int steps, float temperature,
                                 const int32_t* path, const int32_t* path_len, int path_stride, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_trace_decision, dim3((n + 127) / 128), dim3(128), 0, st, tr, row, ids, n, mode, choice, u, sum_G, sum_terms, probs,
                       steps, temperature, path, path_len, path_stride);
}

// One workgroup = one deciding slot i of game ids[i].  The history of the decision: H_act [rows][h_slots][max_depth], H_len and H_active
// [rows][h_slots]; the explored paths of slot i are the rows r < n_iter with H_active[r][i] != 0, cut to H_len[r][i] (and to max_depth).
// The walker starts at (tx, ty) = (int(s[5]), int(s[4])), clamped to 0..31 (a NaN starts at 0), and takes every action `jumps` times;
// a move that happens adds 1 to count[tx][ty].  The counters are integers added with LDS atomics, so the result does not depend on the
// order of the rows; mask = float(count) / float(max count), all zeros when nothing was counted.
constexpr int MASK_THREADS = 256;
__device__ __forceinline__ int mask_start(float f) { return f >= 0.0f ? (f <= 31.0f ? (int)f : 31) : 0; }
__global__ void __launch_bounds__(MASK_THREADS) k_agent_plan_mask(const int32_t* ids, int E, const float* state, const int32_t* H_act,
                                                                  const int32_t* H_len, const uint8_t* H_active, int n_iter, int h_slots,
                                                                  int max_depth, int jumps, float* mask) {
    __shared__ int count[1024];
    __shared__ int top;
    const int i = blockIdx.x;
    const int g = ids[i];
    if (g < 0 || g >= E) return;                                     // memory safety only (the same in every thread of the workgroup)
    for (int c = threadIdx.x; c < 1024; c += MASK_THREADS) count[c] = 0;
    if (threadIdx.x == 0) top = 0;
    __syncthreads();
    const int x0 = mask_start(state[(size_t)g * 7 + 5]), y0 = mask_start(state[(size_t)g * 7 + 4]);
    for (int r = threadIdx.x; r < n_iter; r += MASK_THREADS) {
        const size_t hr = (size_t)r * h_slots + i;
        if (!H_active[hr]) continue;
        int len = H_len[hr];
        len = len > max_depth ? max_depth : len;
        int tx = x0, ty = y0;
        for (int j = 0; j < len; ++j) {
            const int act = H_act[hr * max_depth + j];
            for (int k = 0; k < jumps; ++k) {
                bool moved = false;
                if (act == 0) { if (tx < 31) { ++tx; moved = true; } }
                else if (act == 1) { if (tx > 0) { --tx; moved = true; } }
                else if (act == 2) { if (ty < 31) { ++ty; moved = true; } }
                else if (act == 3) { if (ty > 0) { --ty; moved = true; } }
                if (!moved) break;                                   // blocked (or no action of the four): the repeats of it are blocked too
                atomicAdd(&count[tx * 32 + ty], 1);
            }
        }
    }
    __syncthreads();
    int mx = 0;
    for (int c = threadIdx.x; c < 1024; c += MASK_THREADS) mx = count[c] > mx ? count[c] : mx;
    atomicMax(&top, mx);
    __syncthreads();
    const float ftop = (float)top;
    for (int c = threadIdx.x; c < 1024; c += MASK_THREADS)
        mask[(size_t)g * 1024 + c] = top > 0 ? (float)count[c] / ftop : 0.0f;
}
void launch_agent_plan_mask(const int32_t* ids, int n, int E, const float* state, const int32_t* H_act, const int32_t* H_len,
                            const uint8_t* H_active, int n_iter, int h_slots, int max_depth, int jumps, float* mask, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_plan_mask, dim3(n), dim3(MASK_THREADS), 0, st, ids, E, state, H_act, H_len, H_active, n_iter, h_slots, max_depth,
                       jumps, mask);
}

// One workgroup = one recorded frame i (of game ids[i] when a mask is laid over it).  frames [n][64][64] is efe_env_render's output;
// rows 59..62 of column 31 become 1.0, the game's mask [32][32] is added onto rows and columns 16..47, and the pixel is
// uint8(min(trunc(v * 255), 255)) with NaN -> 0 (and a negative value, which no frame holds, -> 0).
__global__ void __launch_bounds__(256) k_agent_view(const float* frames, const float* mask, const int32_t* ids, int E, uint8_t* view) {
    const int i = blockIdx.x;
    int g = 0;
    if (mask) {
        g = ids[i];
        if (g < 0 || g >= E) return;                                 // memory safety only
    }
    for (int px = threadIdx.x; px < 4096; px += 256) {
        const int y = px >> 6, x = px & 63;
        float v = frames[(size_t)i * 4096 + px];
        if (x == 31 && y >= 59 && y <= 62) v = 1.0f;
        if (mask && y >= 16 && y < 48 && x >= 16 && x < 48) v = v + mask[(size_t)g * 1024 + (y - 16) * 32 + (x - 16)];
        float s = truncf(v * 255.0f);
        s = s < 255.0f ? s : 255.0f;                                 // (a NaN fails the comparison and becomes 255 here, 0 below)
        view[(size_t)i * 4096 + px] = (v != v || s < 0.0f) ? (uint8_t)0 : (uint8_t)(int)s;
    }
}
void launch_agent_view(const float* frames, const float* mask, const int32_t* ids, int n, int E, uint8_t* view, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_view, dim3(n), dim3(256), 0, st, frames, mask, ids, E, view);
}

}  // namespace efe
