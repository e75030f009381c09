// The two ends of an `mcts` decision of the agent loop on the device, so that a decision needs no host round trip of its own:
//
//   k_agent_mcts_root   : the beginning (the reference's mcts.py:166-170 for every deciding game) -- the habit shortcut
//                         `use_habit and max(Qpi) - mean(Qpi) > threshold`, whose action is drawn from Qpi by k_agent_choose's AGENT_PROBS rule
//                         with the SAME key as every other method's action uniform (TAG_AGENT, global game, stream 0, the tick), and the
//                         planner's liveness flags
//   k_agent_mcts_enqueue: the end (Node.action_selection, mcts.py:98-128, plus test_demo.py:167-170) -- the most-visited path of the
//                         slot's tree, trimmed, written into the game's queue with every action `jumps` times
//
// One thread = one deciding SLOT i (the planner's tree arrays are slot-indexed), which belongs to game ids[i] (the queue is game-indexed).
// fp32, mcts.hip's conventions: sums left to right, torch's NaN rules for max / argmax.
#include "kernels.h"

namespace efe {

// Slot i of n.  Qpi [n][A], A = 3 or 4 (the host has checked).  In this order:
//   a Qpi row that holds a NaN, an infinity or a negative entry -> choice -1, empty queue, decided 1, active 0 (k_agent_choose's failure rule)
//   use_habit and thr > threshold, thr = max(Qpi) - (sum left to right) / A -> choice = the draw, queue = choice x jumps, decided 1, active 0
//   otherwise                                                             -> choice -2, the queue is not touched, decided 0, active 1
// The draw: cdf = cumsum(Qpi) / cumsum(Qpi)[A - 1], the first edge above u; u == 1.0 -> the last action with p > 0 (none: -1, empty queue).
__global__ void __launch_bounds__(128) k_agent_mcts_root(const AgentState a, const int32_t* ids, int n, const float* Qpi, int A, int use_habit,
                                                         float threshold, int jumps, uint32_t k0, uint32_t k1, uint32_t stage,
                                                         uint32_t game_offset, const float* u_inj, uint8_t* active, uint8_t* decided,
                                                         int32_t* choice, float* u_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int g = ids[i];
    if (g < 0 || g >= a.E) return;                                   // memory safety only: efe_agent_need writes ids in range
    float p[4];
    for (int k = 0; k < 4; ++k) p[k] = k < A ? Qpi[(size_t)i * A + k] : 0.0f;       // (a fourth entry of 0 changes neither the cdf nor the draw)
    const float u = u_inj ? u_inj[i] : u01(noise_words(k0, k1, TAG_AGENT, 0u, game_offset + (uint32_t)g, 0u, stage).x);
    if (u_out) u_out[i] = u;
    bool ok = true;
    for (int k = 0; k < 4; ++k) ok = ok && p[k] >= 0.0f && p[k] <= 3.402823466e+38f;      // false for NaN, a negative entry and inf
    float mx = p[0], sum = p[0];
    for (int k = 1; k < 4; ++k)
        if (k < A) { mx = p[k] > mx ? p[k] : mx; sum = sum + p[k]; }
    const float thr = mx - sum / (float)A;
    int c = -2, len = 0;
    bool dec = false;
    if (!ok) { c = -1; dec = true; }
    else if (use_habit && thr > threshold) {
        float cdf[4];
        cdf[0] = p[0];
        for (int k = 1; k < 4; ++k) cdf[k] = cdf[k - 1] + p[k];
        const float last = cdf[3];
        c = -1;
        for (int k = 3; k >= 0; --k) if (cdf[k] / last > u) c = k;   // the first edge above u
        if (c < 0)                                                   // u == 1.0
            for (int k = 0; k < 4; ++k) if (p[k] > 0.0f) c = k;
        dec = true;
        len = c < 0 ? 0 : jumps;
    }
    choice[i] = c;
    decided[i] = dec ? 1 : 0;
    active[i] = dec ? 0 : 1;
    if (!dec) return;
    int32_t* q = a.queue + (size_t)g * a.cap;
    for (int k = 0; k < len; ++k) q[k] = c;
    a.head[g] = 0;
    a.len[g] = len;
}
void launch_agent_mcts_root(const AgentState& a, const int32_t* ids, int n, const float* Qpi, int A, int use_habit, float threshold, int jumps,
                            uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, const float* u, uint8_t* active, uint8_t* decided,
                            int32_t* choice, float* u_out, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_mcts_root, dim3((n + 127) / 128), dim3(128), 0, st, a, ids, n, Qpi, A, use_habit, threshold, jumps, k0, k1, stage,
                       game_offset, u, active, decided, choice, u_out);
}

// Slot i of n with decided[i] == 0 (the others are not touched at all).  The walk is Node.action_selection's: from the root, the argmax of the
// visit counts N (first index on ties), down to the first node whose first child is missing.  The trimming of mcts.py:113-128 reads the
// visited actions once, left to right, and looks one action ahead: it runs here WHILE the walk goes on, with the one action it has not yet
// decided about held back (`pend`) -- a cancelling pair (A = 4: up / down, left / right; A = 3: 1 / 2) drops both, anything else emits the
// held action; what is still held when the walk ends is dropped (the loop stops one short of the last visited action).  So there is no
// per-thread path array.  The walk is cut at max_depth actions and at a child index outside [0, cap) (memory safety only: the planner's
// trees are shallower than max_depth = repeats + 2 and its indices in range), hence at most max_depth - 1 actions are emitted.
__global__ void __launch_bounds__(128) k_agent_mcts_enqueue(const AgentState a, const MctsTree t, const int32_t* ids, int n, const uint8_t* decided,
                                                            int max_depth, int jumps, int32_t* path_out, int32_t* path_len_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (decided[i]) return;
    const int g = ids[i];
    if (g < 0 || g >= a.E) return;                                   // memory safety only
    const int A = t.A;
    int32_t* q = a.queue + (size_t)g * a.cap;
    int node = 0, out = 0, pend = -1;
    for (int d = 0; d < max_depth; ++d) {
        const size_t o = ((size_t)i * t.cap + node) * A;
        float nv[4];
        for (int k = 0; k < 4; ++k) nv[k] = k < A ? t.N[o + k] : 0.0f;
        const int act = A == 4 ? argmax_nan_first(nv, 4) : argmax_nan_first(nv, 3);
        if (pend >= 0 && (A == 4 ? (pend ^ 1) == act : pend + act == 3)) pend = -1;        // a cancelling pair: both are dropped
        else {
            if (pend >= 0) {
                for (int r = 0; r < jumps; ++r) q[out * jumps + r] = pend;
                if (path_out) path_out[(size_t)i * max_depth + out] = pend;
                ++out;
            }
            pend = act;
        }
        node = t.child[o + act];
        if (node < 0 || node >= t.cap) break;
        if (t.child[((size_t)i * t.cap + node) * A] < 0) break;      // the node just reached has no children: the walk ends
    }
    a.head[g] = 0;
    a.len[g] = out * jumps;
    if (path_len_out) path_len_out[i] = out;
}
void launch_agent_mcts_enqueue(const AgentState& a, const MctsTree& t, const int32_t* ids, int n, const uint8_t* decided, int max_depth, int jumps,
                               int32_t* path_out, int32_t* path_len_out, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_agent_mcts_enqueue, dim3((n + 127) / 128), dim3(128), 0, st, a, t, ids, n, decided, max_depth, jumps, path_out, path_len_out);
}

}  // namespace efe
