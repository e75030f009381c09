// Per-game control state of the observe-plan-act loop (the loop body of the reference's test_demo.py:118-204) on the device, batched over
// games: an action queue [E][cap] with a head and a length per game (test_demo.py's `executing_steps`), the number of reward crossings
// and the sum of the rewards received.  The last two exist because new_image restarts s[6] at 0 on every crossing (the port quirk that
// env_tick_move replicates), so the score the reference prints is not the task reward.
//
//   k_agent_need   : which games decide this tick (`len(executing_steps) == 0`, :131) as an ascending list + its count
//   k_agent_choose : the draw of :152-184 -- softmax with a temperature and WITHOUT max-subtraction, np.random.choice's inverse CDF,
//                    and the `except: "Not executing anything"` of :185-187 for a distribution that is not one
//   k_agent_enqueue: explicit action lists (the planner's path, :167-170), each action `jumps` times
//   k_agent_act    : :189-204 -- the head action for ONE tick of pi_to_action; a crossing drops the rest of the queue
//
// One thread = one game, as in k_env_*.  A queue is kept normalised: head == 0 whenever len == 0, and choose / enqueue write from slot 0,
// so equal histories give equal bytes.
#include "kernels.h"

namespace efe {

// The games whose queue is empty, in ascending order, and how many there are.  ONE workgroup walks the games in chunks of its size; inside
// a chunk the slot of a game is the number of empty queues before it (wave ballot + the wave totals in LDS), so the list is a function of
// the queue lengths alone: no atomic, no arrival order.  Entries of ids at and beyond *count are not written.
constexpr int NEED_THREADS = 1024;
__global__ void __launch_bounds__(NEED_THREADS) k_agent_need(const AgentState a, int32_t* ids, int32_t* count) {
    __shared__ int wave_total[NEED_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;                                                    // empty queues in the chunks before this one (the same in every thread)
    for (int e0 = 0; e0 < a.E; e0 += NEED_THREADS) {
        const int e = e0 + (int)threadIdx.x;
        const bool empty = e < a.E && a.len[e] == 0;
        const unsigned long long votes = __ballot(empty);
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < NEED_THREADS / 64; ++w) {
            const int n = wave_total[w];
            if (w < wave) before += n;
            total += n;
        }
        if (empty) ids[base + before + __popcll(votes & ((1ull << lane) - 1ull))] = e;
        base += total;
        __syncthreads();                                             // wave_total is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *count = base;
}
void launch_agent_need(const AgentState& a, int32_t* ids, int32_t* count, hipStream_t st) {
    hipLaunchKernelGGL(k_agent_need, dim3(1), dim3(NEED_THREADS), 0, st, a, ids, count);
}

// Deciding game i (of n) is game ids[i].  fp32 in the order of test_demo.py:152-159 (numpy float32 arrays throughout):
//   ai : softmax(-G),              G     = sum_G / steps                          -> x = -(sum_G / steps)
//   t1 : softmax(-term0),          term0 = -sum_terms[0] / steps                  -> x = sum_terms[0] / steps
//   t12: softmax(-(term0 + term1)), term1 = sum_terms[1] / steps                  -> x = sum_terms[0] / steps - sum_terms[1] / steps
//   p = exp(x / T) / sum exp(x / T), the sum left to right, no max-subtraction: an overflow is inf / inf, an underflow of all four 0 / 0.
// np.random.choice(4, p=p): refuses a p that holds a NaN or a negative entry (-> choice -1, empty queue: the game neither moves nor ticks
// and decides again); otherwise cdf = cumsum(p) / cumsum(p)[-1] and the draw is the first edge ABOVE u (searchsorted, side = 'right').
// numpy's u lies in [0, 1); u01 can round to exactly 1.0, above which no edge lies: the draw is then the last action with p > 0.
__global__ void __launch_bounds__(128) k_agent_choose(const AgentState a, const int32_t* ids, int n, int mode, const float* sum_G,
                                                      const float* sum_terms, const float* probs, int steps, float temperature, int repeat,
                                                      uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, const float* u_inj,
                                                      int32_t* choice, float* u_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = ids[i];
    if (g < 0 || g >= a.E) return;                                   // memory safety only: efe_agent_need writes ids in range
    float p[4];
    agent_probs(mode, i, n, sum_G, sum_terms, probs, steps, temperature, p);
    const float u = u_inj ? u_inj[i] : u01(noise_words(k0, k1, TAG_AGENT, 0u, game_offset + (uint32_t)g, 0u, stage).x);
    if (u_out) u_out[i] = u;
    bool ok = true;
    for (int k = 0; k < 4; ++k) ok = ok && p[k] >= 0.0f && p[k] <= 3.402823466e+38f;      // false for NaN, a negative entry and inf
    int c = -1;
    if (ok) {
        float cdf[4];
        cdf[0] = p[0];
        for (int k = 1; k < 4; ++k) cdf[k] = cdf[k - 1] + p[k];
        const float last = cdf[3];
        for (int k = 3; k >= 0; --k) if (cdf[k] / last > u) c = k;   // the first edge above u
        if (c < 0)                                                   // u == 1.0
            for (int k = 0; k < 4; ++k) if (p[k] > 0.0f) c = k;
    }
    choice[i] = c;
    int32_t* q = a.queue + (size_t)g * a.cap;
    const int len = c < 0 ? 0 : repeat;
    for (int k = 0; k < len; ++k) q[k] = c;
    a.head[g] = 0;
    a.len[g] = len;
}
void launch_agent_choose(const AgentState& a, const int32_t* ids, int n, int mode, const float* sum_G, const float* sum_terms, const float* probs,
                         int steps, float temperature, int repeat, uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, const float* u,
                         int32_t* choice, float* u_out, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_choose, dim3((n + 127) / 128), dim3(128), 0, st, a, ids, n, mode, sum_G, sum_terms, probs, steps, temperature,
                       repeat, k0, k1, stage, game_offset, u, choice, u_out);
}

// queue of game ids[i] = actions[i][0 .. lengths[i]), each `jumps` times (lengths are clamped to [0, L]; the host has checked L * jumps <= cap)
__global__ void __launch_bounds__(128) k_agent_enqueue(const AgentState a, const int32_t* ids, int n, const int32_t* actions,
                                                       const int32_t* lengths, int L, int jumps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = ids[i];
    if (g < 0 || g >= a.E) return;                                   // memory safety only
    int len = lengths[i];
    len = len < 0 ? 0 : len > L ? L : len;
    int32_t* q = a.queue + (size_t)g * a.cap;
    for (int j = 0; j < len; ++j) {
        const int32_t act = actions[(size_t)i * L + j];
        for (int r = 0; r < jumps; ++r) q[j * jumps + r] = act;
    }
    a.head[g] = 0;
    a.len[g] = len * jumps;
}
void launch_agent_enqueue(const AgentState& a, const int32_t* ids, int n, const int32_t* actions, const int32_t* lengths, int L, int jumps, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_enqueue, dim3((n + 127) / 128), dim3(128), 0, st, a, ids, n, actions, lengths, L, jumps);
}

// One tick of every game that has something queued (test_demo.py:189-204): env_tick_move is k_env_step's tick, so state, last_r and a
// crossing's new latents are those of efe_env_step(repeats = 1) with the same keys.  A game with an empty queue is not touched at all.
__global__ void __launch_bounds__(128) k_agent_act(const AgentState a, float* state, float* last_r, int32_t* round_changed, uint32_t k0, uint32_t k1,
                                                   uint32_t stage, uint32_t game_offset) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const int len = a.len[e], head = a.head[e];
    if (len < 1 || head < 0 || head + len > a.cap) {                 // empty (the range test is memory safety only: the kernels keep head + len <= cap)
        if (round_changed) round_changed[e] = 0;
        return;
    }
    const int pi = a.queue[(size_t)e * a.cap + head];
    float r = last_r[e];
    const bool changed = env_tick_move(state + (size_t)e * 7, r, pi, k0, k1, game_offset + (uint32_t)e, stage);
    last_r[e] = r;
    if (changed) {
        a.crossings[e] += 1;
        a.reward_sum[e] += r;                                        // r is the reward of this crossing (game_environment.py:125-133)
    }
    const int left = changed ? 0 : len - 1;
    a.len[e] = left;
    a.head[e] = left ? head + 1 : 0;
    if (round_changed) round_changed[e] = changed ? 1 : 0;
}
void launch_agent_act(const AgentState& a, float* state, float* last_r, int32_t* round_changed, uint32_t k0, uint32_t k1, uint32_t stage,
                      uint32_t game_offset, hipStream_t st) {
    hipLaunchKernelGGL(k_agent_act, dim3((a.E + 127) / 128), dim3(128), 0, st, a, state, last_r, round_changed, k0, k1, stage, game_offset);
}

}  // namespace efe
