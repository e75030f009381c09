// Host side of the engine, the inference entry points: the network level (one network per call) and the EFE level (calculate_G, rollouts,
// trajectories, the habit-policy simulation, the action posterior), on the runners of engine_forward.hip.
#include "engine.h"

namespace {

// the row set of a call (efe_rows; NULL = every row, identity)
struct RowSet { const uint8_t* mask; const int32_t* ids; int div; };
int row_set(efe_ctx* ctx, const efe_rows* rows, int n_rows, int fixed_div, RowSet& out, const char* who, hipStream_t st) {
    if (!rows) { out = RowSet{nullptr, nullptr, fixed_div > 0 ? fixed_div : 1}; return 0; }
    const int div = fixed_div > 0 ? fixed_div : rows->rows_per_entry;
    if (div < 1 || ((rows->mask || rows->ids) && n_rows % div != 0)) return ctx->fail(std::string(who) + ": efe_rows.rows_per_entry must divide the row count");
    const int n_entries = n_rows / div;
    if (rows->n_total < 0 || (rows->n_total > 0 && n_entries > rows->n_total))
        return ctx->fail(std::string(who) + ": the call has " + std::to_string(n_entries) + " entries, efe_rows.n_total says " + std::to_string(rows->n_total));
    if (ctx->check_rows && rows->ids && rows->n_total > 0) {          // development option: ids range-checked on the host (synchronises)
        std::vector<int32_t> hid((size_t)n_entries);
        if (hipMemcpyAsync(hid.data(), rows->ids, (size_t)n_entries * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return ctx->fail(std::string(who) + ": check_rows could not read efe_rows.ids");
        for (int i = 0; i < n_entries; ++i)
            if (hid[(size_t)i] < 0 || hid[(size_t)i] >= rows->n_total)
                return ctx->fail(std::string(who) + ": efe_rows.ids[" + std::to_string(i) + "] = " + std::to_string(hid[(size_t)i]) + " is outside [0, n_total = " + std::to_string(rows->n_total) + ")");
    }
    out = RowSet{rows->mask, rows->ids, div};
    return 0;
}

// the noise of the single-group pass (pass, sample) of a call over the row set rs (rows == NULL: exactly pass_noise)
NoiseCfg pass_noise_rows(const efe_noise* nz, uint32_t pass, uint32_t sample, int M, const efe_rows* rows, const RowSet& rs) {
    if (!rows) return pass_noise(nz, pass, sample, M);
    return make_noise((uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), M, nz->row_offset, GroupMap{1, 1, {pass, 0, 0}, nz->stage, sample}, rs.ids, rs.div, rs.mask);
}

// `who`: the entry point the caller used; every refusal names it
int encoder_call(efe_ctx* ctx, const char* who, const float* o, int M, const efe_noise* nz, const float* eps, const efe_rows* rows, float* s,
                 float* mean, float* logvar, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!o || !nz || M < 1) return ctx->fail(std::string(who) + ": bad arguments");
    if (rows && ctx->generic) return ctx->fail("efe_encoder_rows: a row set needs the 1 x 64 x 64 geometry (the generic-geometry path has no row form)");
    RowSet rs;
    if (row_set(ctx, rows, M, 0, rs, "efe_encoder_rows", st)) return 1;
    float* enc = ctx->allocT<float>((size_t)M * 32);
    if (!enc) return 1;
    const NoiseCfg nc = pass_noise_rows(nz, nz->pass, nz->sample, M, rows, rs);
    if (ctx->generic) {
        float* o8 = ctx->allocT<float>((size_t)M * ctx->img_store);
        if (!o8) return 1;
        launch_to_nhwc4(o, o8, M, ctx->res * ctx->res, ctx->chan, st);
        o = o8;
    }
    if (run_encoder(ctx, o, M, nc, enc, st)) return 1;
    launch_split_enc(enc, mean, logvar, M, st);
    if (s) launch_root_post_rows(enc, nullptr, eps, nullptr, s, M, 0, nc.k0, nc.k1, nz->pass, nz->sample, nz->stage, nz->row_offset, ctx->pi_dim, rs.ids, rs.div, st);
    return call.finish();
}

int rollout_call(efe_ctx* ctx, const char* who, const float* o, const float* pi, int M, int steps, int samples, int calc_mean, int per_stage_mean,
                 const efe_noise* nz, const float* eps, const efe_rows* rows, float* sum_G, float* sum_terms, float* po1, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!o || !pi || !nz || !sum_G || M < 1 || steps < 1 || samples < 1 || samples > 65535) return ctx->fail(std::string(who) + ": bad arguments");
    if (rows && ctx->generic) return ctx->fail("efe_rollout_rows: a row set needs the 1 x 64 x 64 geometry (the generic-geometry path has no row form)");
    RowSet rs;
    if (row_set(ctx, rows, M, 0, rs, "efe_rollout_rows", st)) return 1;
    const uint32_t k0 = (uint32_t)nz->seed, k1 = (uint32_t)(nz->seed >> 32);
    const RolloutPlan plan = rollout_plan(ctx, M);
    float* enc0 = ctx->allocT<float>(plan.enc0);
    float* x = ctx->allocT<float>(plan.x);
    if (!enc0 || !x) return 1;
    {   // root encode + reparameterize (torchmodel.py:228-234)
        if (ctx->generic) {
            float* o8 = ctx->allocT<float>(plan.o8);
            if (!o8) return 1;
            launch_to_nhwc4(o, o8, M, ctx->res * ctx->res, ctx->chan, st);
            o = o8;
        }
        if (run_encoder(ctx, o, M, pass_noise_rows(nz, PASS_ROOT, 0, M, rows, rs), enc0, st)) return 1;
        launch_root_post_rows(enc0, pi, eps, x, nullptr, M, calc_mean ? 1 : 0, k0, k1, PASS_ROOT, 0, nz->stage, nz->row_offset, ctx->pi_dim, rs.ids, rs.div, st);
    }
    const int mean_mode = (per_stage_mean && calc_mean) ? 1 : 0;
    CoreIO io{};
    io.x0 = x; io.R = M; io.D = steps; io.S = mean_mode ? 1 : samples; io.mean_mode = mean_mode; io.carry_mean = calc_mean ? 1 : 0;
    io.k0 = k0; io.k1 = k1; io.stage0 = nz->stage; io.row_offset = nz->row_offset;
    io.eps = eps ? eps + (size_t)M * 10 : nullptr;
    io.G = sum_G; io.terms = sum_terms; io.po1 = po1;
    io.mask = rs.mask; io.ids = rs.ids; io.mask_div = rs.div;
    if (run_core(ctx, io, st)) return 1;
    return call.finish();
}

int trajectory_impl(efe_ctx* ctx, const float* s0_traj, const float* ps1_traj, const float* mean_traj, const float* lv_traj,
                    const float* pi0_traj, int T, uint32_t k0, uint32_t k1, uint32_t stage, uint32_t row_offset,
                    const float* eps, float* G, const uint8_t* mask, const int32_t* ids, int mask_div, float* pre_tr, hipStream_t st) {
    float* x = ctx->allocT<float>((size_t)T * 16);
    if (!x) return 1;
    if (!pre_tr) launch_pack_x(pi0_traj, s0_traj, x, T, ctx->pi_dim, S_DIM, st);       // (the transition input: not needed when k_sim_chain has run both transitions)
    CoreIO io{};
    io.x0 = x; io.R = T; io.D = 1; io.S = 1; io.mean_mode = 0; io.carry_mean = 0;
    io.k0 = k0; io.k1 = k1; io.stage0 = stage; io.row_offset = row_offset; io.eps = eps;
    io.given_ps1 = ps1_traj; io.given_mean = mean_traj; io.given_logvar = lv_traj;
    io.G = G; io.mask = mask; io.ids = ids; io.mask_div = mask_div; io.pre_tr = pre_tr;
    return run_core(ctx, io, st);
}

}  // namespace

extern "C" {

// ---- network level -------------------------------------------------------------------------------------
int efe_transition(efe_ctx* ctx, const float* pi, const float* s0, int M, const efe_noise* nz, const float* eps,
                   float* ps1, float* mean, float* logvar, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!pi || !s0 || !nz || M < 1) return ctx->fail("efe_transition: bad arguments");
    float* x = ctx->allocT<float>((size_t)M * 16);
    float* tr = ctx->allocT<float>((size_t)M * 32);
    if (!x || !tr) return 1;
    launch_pack_x(pi, s0, x, M, ctx->pi_dim, S_DIM, st);
    const NoiseCfg nc = pass_noise(nz, nz->pass, nz->sample, M);
    if (run_mid(ctx, x, 0, M, tr, nc, st)) return 1;
    launch_split_enc(tr, mean, logvar, M, st);
    if (ps1) launch_root_post(tr, nullptr, eps, nullptr, ps1, M, 0, nc.k0, nc.k1, nz->pass, nz->sample, nz->stage, nz->row_offset, ctx->pi_dim, st);
    return call.finish();
}

int efe_decoder(efe_ctx* ctx, const float* s, int M, const efe_noise* nz, float* po, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s || !nz || !po || M < 1) return ctx->fail("efe_decoder: bad arguments");
    float* x = ctx->allocT<float>((size_t)M * 16);
    float* val = ctx->allocT<float>((size_t)M * 4);        // (quarter sums when the launch is split; unused by this entry point)
    if (!x || !val) return 1;
    launch_pad16(s, x, M, S_DIM, st);
    const NoiseCfg nc = pass_noise(nz, nz->pass, nz->sample, M);
    if (ctx->generic) {            // the generic path stores NHWC4 images: convert to the NCHW the API returns
        float* tmp = ctx->allocT<float>((size_t)M * ctx->img_store);
        if (!tmp) return 1;
        if (run_decoder(ctx, x, M, nc, 0, 1, val, tmp, st)) return 1;
        launch_to_nchw(tmp, po, M, ctx->res * ctx->res, ctx->chan, st);
    } else if (run_decoder(ctx, x, M, nc, 0, 1, val, po, st)) return 1;
    return call.finish();
}

int efe_encoder(efe_ctx* ctx, const float* o, int M, const efe_noise* nz, const float* eps, float* s, float* mean, float* logvar, void* stream) {
    return encoder_call(ctx, "efe_encoder", o, M, nz, eps, nullptr, s, mean, logvar, stream);
}

int efe_habit(efe_ctx* ctx, const float* s, int M, float* logits, float* q, float* logq, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s || M < 1) return ctx->fail("efe_habit: bad arguments");
    float* x = ctx->allocT<float>((size_t)M * 16);
    float* l32 = ctx->allocT<float>((size_t)M * 32);
    if (!x || !l32) return 1;
    launch_pad16(s, x, M, S_DIM, st);
    if (run_habit(ctx, x, M, l32, st)) return 1;
    launch_softmax4(l32, logits, q, logq, M, ctx->pi_dim, st);
    return call.finish();
}

int efe_check_reward(efe_ctx* ctx, const float* o, int M, float* out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!o || !out || M < 1) return ctx->fail("efe_check_reward: bad arguments");
    if (ctx->generic) launch_check_reward_g(o, out, M, ctx->chan, ctx->res, ctx->res, (int)ctx->reward_intent, (hipStream_t)stream);
    else launch_check_reward(o, out, M, (int)ctx->reward_intent, (hipStream_t)stream);
    return call.finish();
}

int efe_reparameterize(efe_ctx* ctx, const float* mean, const float* logvar, int M, int n, const efe_noise* nz, const float* eps,
                       float* out, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!mean || !logvar || !nz || !out || M < 1 || n < 1) return ctx->fail("efe_reparameterize: bad arguments");
    launch_reparam(mean, logvar, eps, out, M, n, (uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->pass, nz->sample, nz->stage,
                   nz->row_offset, (hipStream_t)stream);
    return call.finish();
}

// ---- EFE level -----------------------------------------------------------------------------------------
int efe_calculate_g(efe_ctx* ctx, const float* s0, const float* pi0, int M, int samples, int mean_mode, const efe_noise* nz,
                    const float* eps, float* G, float* terms, float* ps1, float* ps1_mean, float* po1, float* t2parts, void* stream) {
    return efe_calculate_g_rows(ctx, s0, pi0, M, samples, mean_mode, nz, eps, nullptr, G, terms, ps1, ps1_mean, po1, t2parts, stream);
}

int efe_calculate_g_rows(efe_ctx* ctx, const float* s0, const float* pi0, int M, int samples, int mean_mode, const efe_noise* nz,
                         const float* eps, const efe_rows* rows, float* G, float* terms, float* ps1, float* ps1_mean, float* po1,
                         float* t2parts, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s0 || !pi0 || !nz || !G || M < 1 || samples < 1 || samples > 65535) return ctx->fail("efe_calculate_g: bad arguments");
    float* x = ctx->allocT<float>((size_t)M * 16);
    if (!x) return 1;
    launch_pack_x(pi0, s0, x, M, ctx->pi_dim, S_DIM, st);
    CoreIO io{};
    io.x0 = x; io.R = M; io.D = 1; io.S = mean_mode ? 1 : samples; io.mean_mode = mean_mode; io.carry_mean = 0;
    io.k0 = (uint32_t)nz->seed; io.k1 = (uint32_t)(nz->seed >> 32); io.stage0 = nz->stage; io.row_offset = nz->row_offset;
    io.eps = eps; io.G = G; io.terms = terms; io.ps1 = ps1; io.ps1_mean = ps1_mean; io.po1 = po1; io.t2parts = t2parts;
    RowSet rs;
    if (row_set(ctx, rows, M, 0, rs, "efe_calculate_g_rows", st)) return 1;
    io.mask = rs.mask; io.ids = rs.ids; io.mask_div = rs.div;
    if (run_core(ctx, io, st)) return 1;
    return call.finish();
}

int efe_encoder_rows(efe_ctx* ctx, const float* o, int M, const efe_noise* nz, const float* eps, const efe_rows* rows, float* s, float* mean,
                     float* logvar, void* stream) {
    return encoder_call(ctx, "efe_encoder_rows", o, M, nz, eps, rows, s, mean, logvar, stream);
}

int efe_rollout(efe_ctx* ctx, const float* o, const float* pi, int M, int steps, int samples, int calc_mean, int per_stage_mean,
                const efe_noise* nz, const float* eps, float* sum_G, float* sum_terms, float* po1, void* stream) {
    return rollout_call(ctx, "efe_rollout", o, pi, M, steps, samples, calc_mean, per_stage_mean, nz, eps, nullptr, sum_G, sum_terms, po1, stream);
}
int efe_rollout_rows(efe_ctx* ctx, const float* o, const float* pi, int M, int steps, int samples, int calc_mean, int per_stage_mean,
                     const efe_noise* nz, const float* eps, const efe_rows* rows, float* sum_G, float* sum_terms, float* po1, void* stream) {
    return rollout_call(ctx, "efe_rollout_rows", o, pi, M, steps, samples, calc_mean, per_stage_mean, nz, eps, rows, sum_G, sum_terms, po1, stream);
}

int efe_trajectory(efe_ctx* ctx, const float* s0_traj, const float* ps1_traj, const float* ps1_mean_traj, const float* ps1_logvar_traj,
                   const float* pi0_traj, int T, const efe_noise* nz, const float* eps, float* G, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s0_traj || !ps1_traj || !ps1_mean_traj || !ps1_logvar_traj || !pi0_traj || !nz || !G || T < 1)
        return ctx->fail("efe_trajectory: bad arguments");
    if (trajectory_impl(ctx, s0_traj, ps1_traj, ps1_mean_traj, ps1_logvar_traj, pi0_traj, T, (uint32_t)nz->seed,
                        (uint32_t)(nz->seed >> 32), nz->stage, nz->row_offset, eps, G, nullptr, nullptr, 1, nullptr, st)) return 1;
    return call.finish();
}

int efe_simulate(efe_ctx* ctx, const float* starting_s, int E, int depth, int use_means, const efe_noise* nz,
                 const float* eps, const float* u, float* G_mean, float* pi0, float* Qpi0, void* stream) {
    return efe_simulate_rows(ctx, starting_s, E, depth, use_means, nz, eps, u, nullptr, G_mean, pi0, Qpi0, stream);
}

int efe_simulate_rows(efe_ctx* ctx, const float* starting_s, int E, int depth, int use_means, const efe_noise* nz,
                      const float* eps, const float* u, const efe_rows* rows, float* G_mean, float* pi0, float* Qpi0, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!starting_s || !nz || !G_mean || !pi0 || E < 1 || depth < 1 || depth > 65535) return ctx->fail("efe_simulate: bad arguments");
    const uint32_t k0 = (uint32_t)nz->seed, k1 = (uint32_t)(nz->seed >> 32);
    const int T = depth;
    RowSet rs;
    if (row_set(ctx, rows, E, 1, rs, "efe_simulate_rows", (hipStream_t)stream)) return 1;      // one episode = one entry
    float* s0t = ctx->allocT<float>((size_t)E * T * 10);
    float* ps1t = ctx->allocT<float>((size_t)E * T * 10);
    float* mt = ctx->allocT<float>((size_t)E * T * 10);
    float* lvt = ctx->allocT<float>((size_t)E * T * 10);
    float* Gt = ctx->allocT<float>((size_t)E * T);
    // the trajectory core's transition rows, written by the chain kernel -- unless the A/B option mid_unfused asks for the layer-by-layer
    // transition: then the trajectory's loop-2 transition goes through run_mid like every other one (the chain kernel keeps its own rollout)
    float* trp = ctx->allocT<float>((size_t)2 * E * T * 32);
    float* pre_tr = ctx->mid_unfused ? nullptr : trp;
    if (!s0t || !ps1t || !mt || !lvt || !Gt || !trp) return 1;
    bool split_launch = false;
    {   // the whole habit-policy rollout (depth x (encode_s, sample, transition, reparameterise)) is one launch (fused.hip)
        SimChainArgs sa{};
        sa.W = ctx->mid16; sa.H = ctx->top16; sa.s0 = starting_s; sa.E = E; sa.T = T; sa.use_means = use_means;
        sa.k0 = k0; sa.k1 = k1; sa.stage = nz->stage; sa.row_offset = nz->row_offset;
        sa.eps_inj = eps; sa.u_inj = u; sa.ids = rs.ids;
        if (ctx->sim_split && (E + SIM_FE - 1) / SIM_FE <= SIM_MAX_SPLIT_GROUPS) {
            // The split form's arrival counters and sticky timeout flag re-arm themselves at the end of a launch.  Whenever the previous
            // split call did not reach its end on the host (an error behind the kernel's enqueue) they are zeroed on the stream first --
            // not before every launch: a 32-byte hipMemsetAsync costs ~25 us of the 400 us a one-episode planner iteration takes.
            sa.xch = ctx->sim_xch; sa.sync = ctx->sim_sync;
            if (ctx->sim_sync_dirty && hipMemsetAsync(ctx->sim_sync, 0, (size_t)SIM_MAX_SPLIT_GROUPS * 4 * sizeof(int), st) != hipSuccess)
                return ctx->fail("efe_simulate: sim_sync memset failed");
            ctx->sim_sync_dirty = true;             // cleared where this call has enqueued everything and found no launch error
            split_launch = true;
        }
        sa.s0_traj = s0t; sa.ps1_traj = ps1t; sa.mean_traj = mt; sa.lv_traj = lvt; sa.pi0 = pi0; sa.Qpi0 = Qpi0; sa.pi_dim = ctx->pi_dim; sa.tr = pre_tr;
        {
            ProfSpan span(ctx, PROF_MID, st);
            launch_sim_chain(sa, st);
        }
        ctx->last_macs += (int64_t)E * T * (2 * ctx->mac_trans + ctx->mac_habit);      // the rollout's transition and the trajectory's loop-2 transition
    }
    if (trajectory_impl(ctx, s0t, ps1t, mt, lvt, pi0, E * T, k0, k1, nz->stage, nz->row_offset * (uint32_t)T,
                        eps ? eps + (size_t)T * E * 10 : nullptr, Gt, rs.mask, rs.ids, T, pre_tr, st)) return 1;     // trajectory row e * T + t belongs to episode slot e
    launch_mean_rows(Gt, G_mean, E, T, st);
    const int rc = call.finish();
    if (rc == 0 && split_launch) ctx->sim_sync_dirty = false;
    return rc;
}

int efe_action_posterior(efe_ctx* ctx, const float* sum_G, int n_groups, int n, float temperature, float* P, float* logP, void* stream) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (!sum_G || !P || !logP || n_groups < 1 || n < 1 || n > 8) return ctx->fail("efe_action_posterior: bad arguments");
    launch_posterior(sum_G, P, logP, n_groups, n, temperature, (hipStream_t)stream);
    return call.finish();
}

}  // extern "C"
