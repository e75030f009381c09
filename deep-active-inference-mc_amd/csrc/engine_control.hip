// Host side of the engine, control: the entry points of the Dynamic-dSprites environment (kernels.hip), the agent's control state
// (agent.hip), the record of its run (agent_trace.hip) and the planner's tree (mcts.hip).  None takes scratch: each checks its arguments
// and launches.
#include "engine.h"

namespace {

int mcts_tree(efe_ctx* ctx, const efe_mcts_tree* t, MctsTree& o) {
    if (!t || !t->W || !t->N || !t->Qpi || !t->child || !t->S || t->E < 1 || t->cap < 1 || t->A < 1 || t->A > 8 || t->s_dim < 1)
        return ctx->fail("efe_mcts: bad tree");
    o = MctsTree{t->W, t->N, t->Qpi, t->child, t->S, t->E, t->cap, t->A, t->s_dim};
    return 0;
}

// ---- agent control state (csrc/agent.hip): every refusal comes before the first launch and names its entry point ----
int agent_state(efe_ctx* ctx, const char* fn, const efe_agent* ag, AgentState& o) {
    if (!ag) return ctx->fail(std::string(fn) + ": agent is NULL");
    if (ag->E < 1) return ctx->fail(std::string(fn) + ": E < 1");
    if (ag->cap < 1) return ctx->fail(std::string(fn) + ": cap < 1");
    if (!ag->queue || !ag->head || !ag->len || !ag->crossings || !ag->reward_sum) return ctx->fail(std::string(fn) + ": a NULL array in efe_agent");
    o = AgentState{ag->queue, ag->head, ag->len, ag->crossings, ag->reward_sum, ag->E, ag->cap};
    return 0;
}

// the record of an agent run (csrc/agent_trace.hip): every array is required, `row` must lie inside the record
int agent_trace(efe_ctx* ctx, const char* fn, const efe_agent_trace* tr, int row, AgentTrace& o) {
    if (!tr) return ctx->fail(std::string(fn) + ": trace is NULL");
    if (tr->E < 1) return ctx->fail(std::string(fn) + ": E < 1");
    if (tr->T < 1 || tr->Lp < 1) return ctx->fail(std::string(fn) + ": T < 1 or Lp < 1");
    if (row < 0 || row >= tr->T) return ctx->fail(std::string(fn) + ": row " + std::to_string(row) + " is outside the record of " + std::to_string(tr->T) + " rows");
    if (!tr->state || !tr->last_r || !tr->action || !tr->queue_len || !tr->decided || !tr->choice || !tr->u || !tr->G || !tr->terms || !tr->probs ||
        !tr->path || !tr->path_len)
        return ctx->fail(std::string(fn) + ": a NULL array in efe_agent_trace");
    o = AgentTrace{tr->state, tr->last_r, tr->action, tr->queue_len, tr->decided, tr->choice, tr->u, tr->G, tr->terms, tr->probs, tr->path,
                   tr->path_len, tr->T, tr->E, tr->Lp};
    return 0;
}

}  // namespace

extern "C" {

int efe_env_reset(efe_ctx* ctx, float* state, float* last_r, int E, const efe_noise* nz, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!state || !last_r || !nz || E < 1) return ctx->fail("efe_env_reset: bad arguments");
    launch_env_reset(state, last_r, E, (uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->stage, nz->row_offset, (hipStream_t)stream);
    return call.finish();
}

int efe_env_new_image(efe_ctx* ctx, float* state, int E, const efe_noise* nz, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!state || !nz || E < 1) return ctx->fail("efe_env_new_image: bad arguments");
    launch_env_new_image(state, E, (uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->stage, nz->row_offset, (hipStream_t)stream);
    return call.finish();
}

int efe_env_step(efe_ctx* ctx, float* state, float* last_r, const int32_t* actions, int E, int repeats, const efe_noise* nz,
                 int32_t* round_changed, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!state || !last_r || !actions || !nz || E < 1 || repeats < 1) return ctx->fail("efe_env_step: bad arguments");
    launch_env_step(state, last_r, actions, round_changed, E, repeats, (uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->stage,
                    nz->row_offset, (hipStream_t)stream);
    return call.finish();
}

int efe_env_render(efe_ctx* ctx, const float* state, const float* last_r, const uint8_t* imgs, int64_t n_imgs, float* frames,
                   int32_t* err, int E, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!state || !last_r || !imgs || !frames || n_imgs < 1 || E < 1) return ctx->fail("efe_env_render: bad arguments");
    launch_env_render(state, last_r, imgs, (long)n_imgs, frames, err, E, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_need(efe_ctx* ctx, const efe_agent* agent, int32_t* ids, int32_t* count, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_need", agent, a)) return 1;
    if (!ids || !count) return ctx->fail("efe_agent_need: ids or count is NULL");
    launch_agent_need(a, ids, count, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_choose(efe_ctx* ctx, const efe_agent* agent, const int32_t* ids, int n, int mode, const float* sum_G, const float* sum_terms,
                     const float* probs, int steps, float temperature, int repeat, const efe_noise* nz, const float* u, int32_t* choice,
                     float* u_out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_choose", agent, a)) return 1;
    if (n < 0 || n > a.E) return ctx->fail("efe_agent_choose: n < 0 or n > E");
    if (mode != EFE_AGENT_AI && mode != EFE_AGENT_T1 && mode != EFE_AGENT_T12 && mode != EFE_AGENT_PROBS)
        return ctx->fail("efe_agent_choose: unknown mode " + std::to_string(mode));
    if (steps < 1) return ctx->fail("efe_agent_choose: steps < 1");
    if (!(temperature > 0.0f) || std::isinf(temperature)) return ctx->fail("efe_agent_choose: the temperature must be finite and positive");
    if (repeat < 1) return ctx->fail("efe_agent_choose: repeat < 1");
    if (repeat > a.cap) return ctx->fail("efe_agent_choose: the queue capacity " + std::to_string(a.cap) + " is smaller than repeat = " + std::to_string(repeat));
    if (!ids || !choice) return ctx->fail("efe_agent_choose: ids or choice is NULL");
    if (!nz && !u) return ctx->fail("efe_agent_choose: neither efe_noise nor injected uniforms");
    if (mode == EFE_AGENT_AI && !sum_G) return ctx->fail("efe_agent_choose: mode ai needs sum_G");
    if ((mode == EFE_AGENT_T1 || mode == EFE_AGENT_T12) && !sum_terms) return ctx->fail("efe_agent_choose: modes t1 and t12 need sum_terms");
    if (mode == EFE_AGENT_PROBS && !probs) return ctx->fail("efe_agent_choose: mode probs needs probs");
    const uint64_t seed = nz ? nz->seed : 0;
    launch_agent_choose(a, ids, n, mode, sum_G, sum_terms, probs, steps, temperature, repeat, (uint32_t)seed, (uint32_t)(seed >> 32),
                        nz ? nz->stage : 0u, nz ? nz->row_offset : 0u, u, choice, u_out, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_enqueue(efe_ctx* ctx, const efe_agent* agent, const int32_t* ids, int n, const int32_t* actions, const int32_t* lengths, int L,
                      int jumps, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_enqueue", agent, a)) return 1;
    if (n < 0 || n > a.E) return ctx->fail("efe_agent_enqueue: n < 0 or n > E");
    if (L < 1 || jumps < 1) return ctx->fail("efe_agent_enqueue: L < 1 or jumps < 1");
    if ((int64_t)L * jumps > a.cap)
        return ctx->fail("efe_agent_enqueue: the queue capacity " + std::to_string(a.cap) + " is smaller than L * jumps = " + std::to_string((int64_t)L * jumps));
    if (!ids || !actions || !lengths) return ctx->fail("efe_agent_enqueue: ids, actions or lengths is NULL");
    launch_agent_enqueue(a, ids, n, actions, lengths, L, jumps, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_act(efe_ctx* ctx, const efe_agent* agent, float* state, float* last_r, const efe_noise* nz, int32_t* round_changed, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_act", agent, a)) return 1;
    if (!state || !last_r || !nz) return ctx->fail("efe_agent_act: state, last_r or efe_noise is NULL");
    launch_agent_act(a, state, last_r, round_changed, (uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->stage, nz->row_offset, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_mcts_root(efe_ctx* ctx, const efe_agent* agent, const int32_t* ids, int n, const float* Qpi, int A, int use_habit, float threshold,
                        int max_depth, int jumps, const efe_noise* nz, const float* u, uint8_t* active, uint8_t* decided, int32_t* choice,
                        float* u_out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_mcts_root", agent, a)) return 1;
    if (n < 0 || n > a.E) return ctx->fail("efe_agent_mcts_root: n < 0 or n > E");
    if (A != 3 && A != 4) return ctx->fail("efe_agent_mcts_root: A = " + std::to_string(A) + ", the path trimming is defined for 3 and 4 actions");
    if (jumps < 1) return ctx->fail("efe_agent_mcts_root: jumps < 1");
    if (max_depth < 1) return ctx->fail("efe_agent_mcts_root: max_depth < 1");
    if ((int64_t)max_depth * jumps > a.cap)
        return ctx->fail("efe_agent_mcts_root: the queue capacity " + std::to_string(a.cap) + " is smaller than max_depth * jumps = " +
                         std::to_string((int64_t)max_depth * jumps) + ", the longest queue this decision could write");
    if (!ids || !Qpi || !active || !decided || !choice) return ctx->fail("efe_agent_mcts_root: ids, Qpi, active, decided or choice is NULL");
    if (!nz && !u) return ctx->fail("efe_agent_mcts_root: neither efe_noise nor injected uniforms");
    const uint64_t seed = nz ? nz->seed : 0;
    launch_agent_mcts_root(a, ids, n, Qpi, A, use_habit ? 1 : 0, threshold, jumps, (uint32_t)seed, (uint32_t)(seed >> 32), nz ? nz->stage : 0u,
                           nz ? nz->row_offset : 0u, u, active, decided, choice, u_out, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_mcts_enqueue(efe_ctx* ctx, const efe_agent* agent, const efe_mcts_tree* tree, const int32_t* ids, int n, const uint8_t* decided,
                           int max_depth, int jumps, int32_t* path_out, int32_t* path_len_out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_mcts_enqueue", agent, a)) return 1;
    if (n < 0 || n > a.E) return ctx->fail("efe_agent_mcts_enqueue: n < 0 or n > E");
    if (!tree) return ctx->fail("efe_agent_mcts_enqueue: tree is NULL");
    if (tree->A != 3 && tree->A != 4)
        return ctx->fail("efe_agent_mcts_enqueue: A = " + std::to_string(tree->A) + ", the path trimming is defined for 3 and 4 actions");
    if (!tree->N || !tree->child) return ctx->fail("efe_agent_mcts_enqueue: N or child of the tree is NULL");
    if (tree->cap < 1 || n > tree->E) return ctx->fail("efe_agent_mcts_enqueue: the tree has cap < 1 or fewer than n slots");
    if (jumps < 1) return ctx->fail("efe_agent_mcts_enqueue: jumps < 1");
    if (max_depth < 1) return ctx->fail("efe_agent_mcts_enqueue: max_depth < 1");
    if ((int64_t)max_depth * jumps > a.cap)
        return ctx->fail("efe_agent_mcts_enqueue: the queue capacity " + std::to_string(a.cap) + " is smaller than max_depth * jumps = " +
                         std::to_string((int64_t)max_depth * jumps) + ", the longest queue this call could write");
    if (!ids || !decided) return ctx->fail("efe_agent_mcts_enqueue: ids or decided is NULL");
    const MctsTree t{tree->W, tree->N, tree->Qpi, tree->child, tree->S, tree->E, tree->cap, tree->A, tree->s_dim};
    launch_agent_mcts_enqueue(a, t, ids, n, decided, max_depth, jumps, path_out, path_len_out, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_trace_tick(efe_ctx* ctx, const efe_agent* agent, const efe_agent_trace* trace, int row, const float* state, const float* last_r,
                         void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentState a; if (agent_state(ctx, "efe_agent_trace_tick", agent, a)) return 1;
    AgentTrace tr; if (agent_trace(ctx, "efe_agent_trace_tick", trace, row, tr)) return 1;
    if (tr.E != a.E) return ctx->fail("efe_agent_trace_tick: the record holds " + std::to_string(tr.E) + " games, the agent " + std::to_string(a.E));
    if (!state || !last_r) return ctx->fail("efe_agent_trace_tick: state or last_r is NULL");
    launch_agent_trace_tick(a, tr, row, state, last_r, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_trace_decision(efe_ctx* ctx, const efe_agent_trace* trace, int row, const int32_t* ids, int n, int mode, const int32_t* choice,
                             const float* u, const float* sum_G, const float* sum_terms, const float* probs, int steps, float temperature,
                             const int32_t* path, const int32_t* path_len, int path_stride, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    AgentTrace tr; if (agent_trace(ctx, "efe_agent_trace_decision", trace, row, tr)) return 1;
    if (n < 0 || n > tr.E) return ctx->fail("efe_agent_trace_decision: n < 0 or n > E");
    if (mode != EFE_AGENT_NONE && mode != EFE_AGENT_AI && mode != EFE_AGENT_T1 && mode != EFE_AGENT_T12 && mode != EFE_AGENT_PROBS)
        return ctx->fail("efe_agent_trace_decision: unknown mode " + std::to_string(mode));
    if (!ids) return ctx->fail("efe_agent_trace_decision: ids is NULL");
    if (mode == EFE_AGENT_AI || mode == EFE_AGENT_T1 || mode == EFE_AGENT_T12) {
        if (!sum_G || !sum_terms) return ctx->fail("efe_agent_trace_decision: modes ai, t1 and t12 need sum_G and sum_terms");
        if (steps < 1) return ctx->fail("efe_agent_trace_decision: steps < 1");
        if (!(temperature > 0.0f) || std::isinf(temperature)) return ctx->fail("efe_agent_trace_decision: the temperature must be finite and positive");
    }
    if (mode == EFE_AGENT_PROBS && !probs) return ctx->fail("efe_agent_trace_decision: mode probs needs probs");
    if ((path != nullptr) != (path_len != nullptr)) return ctx->fail("efe_agent_trace_decision: path and path_len come together");
    if (path && path_stride < 1) return ctx->fail("efe_agent_trace_decision: path_stride < 1");
    launch_agent_trace_decision(tr, row, ids, n, mode, choice, u, sum_G, sum_terms, probs, steps, temperature, path, path_len, path_stride,
                                (hipStream_t)stream);
    return call.finish();
}

int efe_agent_plan_mask(efe_ctx* ctx, const int32_t* ids, int n, int E, const float* state, const int32_t* H_act, const int32_t* H_len,
                        const uint8_t* H_active, int n_iter, int h_slots, int max_depth, int jumps, int A, float* mask, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (E < 1) return ctx->fail("efe_agent_plan_mask: E < 1");
    if (n < 0 || n > E) return ctx->fail("efe_agent_plan_mask: n < 0 or n > E");
    if (A != 4) return ctx->fail("efe_agent_plan_mask: A = " + std::to_string(A) + ", the walk of the mask is defined for 4 actions");
    if (jumps < 1) return ctx->fail("efe_agent_plan_mask: jumps < 1");
    if (max_depth < 1 || n_iter < 0) return ctx->fail("efe_agent_plan_mask: max_depth < 1 or n_iter < 0");
    if (n > h_slots) return ctx->fail("efe_agent_plan_mask: the history has fewer than n slots");
    if (!ids || !state || !H_act || !H_len || !H_active || !mask) return ctx->fail("efe_agent_plan_mask: ids, state, a history array or mask is NULL");
    launch_agent_plan_mask(ids, n, E, state, H_act, H_len, H_active, n_iter, h_slots, max_depth, jumps, mask, (hipStream_t)stream);
    return call.finish();
}

int efe_agent_view(efe_ctx* ctx, const float* frames, const float* mask, const int32_t* ids, int n, int E, uint8_t* view, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (E < 1) return ctx->fail("efe_agent_view: E < 1");
    if (n < 0 || n > E) return ctx->fail("efe_agent_view: n < 0 or n > E");
    if (!frames || !view) return ctx->fail("efe_agent_view: frames or view is NULL");
    if (mask && !ids) return ctx->fail("efe_agent_view: a mask needs ids");
    launch_agent_view(frames, mask, ids, n, E, view, (hipStream_t)stream);
    return call.finish();
}

int efe_mcts_select(efe_ctx* ctx, const efe_mcts_tree* tree, const uint8_t* active, float C, int use_prior, int max_depth,
                    int32_t* path_nodes, int32_t* path_act, int32_t* path_len, int32_t* leaf, float* leaf_s, float* leaf_s_rep,
                    void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    MctsTree t; if (mcts_tree(ctx, tree, t)) return 1;
    if (!active || !path_nodes || !path_act || !path_len || !leaf || !leaf_s || !leaf_s_rep || max_depth < 1)
        return ctx->fail("efe_mcts_select: bad arguments");
    launch_mcts_select(t, active, C, use_prior, max_depth, path_nodes, path_act, path_len, leaf, leaf_s, leaf_s_rep, (hipStream_t)stream);
    return call.finish();
}

int efe_mcts_expand(efe_ctx* ctx, const efe_mcts_tree* tree, int32_t* n_nodes, const int32_t* nodes, const uint8_t* mask, const float* G,
                    const float* ps_next, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    MctsTree t; if (mcts_tree(ctx, tree, t)) return 1;
    if (!n_nodes || !nodes || !mask || !G || !ps_next) return ctx->fail("efe_mcts_expand: bad arguments");
    launch_mcts_expand(t, n_nodes, nodes, mask, G, ps_next, (hipStream_t)stream);
    return call.finish();
}

int efe_mcts_backprop(efe_ctx* ctx, const efe_mcts_tree* tree, const int32_t* path_nodes, const int32_t* path_act, const int32_t* path_len,
                      const int32_t* leaf, const uint8_t* active, const float* sims, int n_sims, const float* q0, int max_depth,
                      float* g_out, uint8_t* active_out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    MctsTree t; if (mcts_tree(ctx, tree, t)) return 1;
    if (!path_nodes || !path_act || !path_len || !leaf || !active || !sims || n_sims < 1 || !q0 || !g_out || !active_out || max_depth < 1)
        return ctx->fail("efe_mcts_backprop: bad arguments");
    launch_mcts_backprop(t, path_nodes, path_act, path_len, leaf, active, sims, n_sims, q0, max_depth, g_out, active_out, (hipStream_t)stream);
    return call.finish();
}

int efe_mcts_step(efe_ctx* ctx, const efe_mcts_tree* tree, const int32_t* prev_path_act, const int32_t* prev_path_len, const float* sims, int n_sims,
                  const float* q0, float* prev_g_out, uint8_t* prev_active_out, uint8_t* active, int32_t* stop_at, int repeat, float threshold,
                  int32_t* n_active, float C, int use_prior, int max_depth, int32_t* path_nodes, int32_t* path_act, int32_t* path_len, int32_t* leaf,
                  float* leaf_s, float* leaf_s_rep, int32_t* prev_n_nodes, const float* prev_G, const float* prev_ps_next, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    MctsTree t; if (mcts_tree(ctx, tree, t)) return 1;
    const int n_exp = (prev_n_nodes != nullptr) + (prev_G != nullptr) + (prev_ps_next != nullptr);
    if (!active || !stop_at || !n_active || !path_nodes || !path_act || !path_len || !leaf || !leaf_s || !leaf_s_rep || max_depth < 1 ||
        (prev_path_len && (!prev_path_act || !sims || n_sims < 1 || !q0 || !prev_g_out || !prev_active_out)) || (n_exp != 0 && n_exp != 3))
        return ctx->fail("efe_mcts_step: bad arguments");
    MctsStepArgs a{prev_path_act, prev_path_len, sims, n_sims, q0, prev_g_out, prev_active_out, active, stop_at, repeat, threshold, n_active,
                   C, use_prior, max_depth, path_nodes, path_act, path_len, leaf, leaf_s, leaf_s_rep, prev_n_nodes, prev_G, prev_ps_next};
    launch_mcts_step(t, a, (hipStream_t)stream);
    return call.finish();
}

int efe_mcts_stop(efe_ctx* ctx, const efe_mcts_tree* tree, uint8_t* active, int32_t* stop_at, int repeat, float threshold,
                  int32_t* n_active, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    MctsTree t; if (mcts_tree(ctx, tree, t)) return 1;
    if (!active || !stop_at || !n_active) return ctx->fail("efe_mcts_stop: bad arguments");
    launch_mcts_stop(t, active, stop_at, repeat, threshold, n_active, (hipStream_t)stream);
    return call.finish();
}

}  // extern "C"
