// Host side of the engine, the training-side free energy (loss.hip): F_top, F_mid and F_down of the reference's compute_loss_* as
// entry points, and the helpers that the gradient calls of engine_train.hip share with them; and the epoch report (eval.hip), which
// reduces their per-row outputs into one row of statistics.
#include "engine.h"

namespace efe {
namespace host {
namespace {

// the observation as the encoder reads it: NCHW as given (dSprites), NHWC4 in scratch (generic geometry)
const float* fe_obs(efe_ctx* ctx, const float* o, int M, hipStream_t st) {
    if (!ctx->generic) return o;
    float* o4 = ctx->allocT<float>((size_t)M * ctx->img_store);
    if (o4) launch_to_nhwc4(o, o4, M, ctx->res * ctx->res, ctx->chan, st);
    return o4;
}
// the decoder over rows [m0, m0 + chunk) per launch group, then k_fe_down on the same rows: scratch is one chunk of images (the arena
// position is put back after every chunk; the stream orders the chunks), and every row's noise key and result is that of a single call
int fe_down(efe_ctx* ctx, const float* dec_in, int M, const NoiseCfg& base, const FeArgs& a, float* po1, hipStream_t st) {
    const int C = (int)std::min<int64_t>(ctx->dec_chunk, M);
    const int HW = ctx->res * ctx->res;
    const bool direct = po1 && !ctx->generic;             // dSprites stores NCHW: the decoder writes the caller's po1
    float* po_s = direct ? nullptr : ctx->allocT<float>((size_t)C * ctx->img_store);
    float* val = ctx->allocT<float>((size_t)C * 4);       // (per-image entropy sums of the decoder epilogue: unused here)
    if ((!direct && !po_s) || !val) return 1;
    for (int m0 = 0; m0 < M; m0 += C) {
        const int c = std::min(C, M - m0);
        const Arena::Mark mark = ctx->arena.mark();
        NoiseCfg nc = base; nc.rows_per_group = c; nc.row_offset = base.row_offset + (uint32_t)m0;
        float* img = po_s ? po_s : po1 + (size_t)m0 * ctx->img_store;
        if (run_decoder(ctx, dec_in + (size_t)m0 * 16, c, nc, 0, 1, val, img, st)) return 1;
        if (ctx->generic && po1) launch_to_nchw(img, po1 + (size_t)m0 * ctx->chan * HW, c, HW, ctx->chan, st);
        launch_fe_down(a, img, m0, c, st);
        ctx->arena.rewind(mark);
    }
    return 0;
}

}  // namespace

// ---- what other host files call (engine.h) -----------------------------------------------------------
int fe_params(efe_ctx* ctx, const efe_fe_params* p, bool derived_ok, const char* who) {
    const std::string w(who);
    if (!p) return ctx->fail(w + ": params is NULL");
    if (p->omega_mode == EFE_OMEGA_ARRAY && !p->omega) return ctx->fail(w + ": omega_mode EFE_OMEGA_ARRAY needs params->omega");
    if (p->omega_mode == EFE_OMEGA_DERIVED && !derived_ok) return ctx->fail(w + ": omega_mode EFE_OMEGA_DERIVED needs kl_pi (efe_free_energy only)");
    if (p->omega_mode < EFE_OMEGA_ARRAY || p->omega_mode > EFE_OMEGA_DERIVED) return ctx->fail(w + ": unknown omega_mode " + std::to_string(p->omega_mode));
    return 0;
}
void fe_omega(FeArgs& a, const efe_fe_params* p) {
    a.omega_mode = p->omega_mode; a.omega_in = p->omega; a.omega_scalar = p->omega_scalar;
    a.oa_a = p->a; a.oa_b = p->b; a.oa_c = p->c; a.oa_d = p->d;
}
FeArgs fe_down_args(efe_ctx* ctx, int M, const float* o1, const float* enc, const float* p1_mean, const float* p1_lv, int p1_ld,
                    const efe_fe_params* p, const float* omega, const efe_fe_out* out) {
    FeArgs a{};
    a.M = M; a.A = ctx->pi_dim;
    a.omega_mode = omega ? 0 : 1; a.omega_in = omega; a.omega_scalar = p->omega_scalar;
    a.q1_mean = enc; a.q1_lv = enc + 10; a.q1_ld = 32; a.p1_mean = p1_mean; a.p1_lv = p1_lv; a.p1_ld = p1_ld;
    a.o1 = o1; a.C = ctx->chan; a.HW = ctx->res * ctx->res; a.nhwc4 = ctx->generic ? 1 : 0;
    a.gamma = p->gamma; a.beta_s = p->beta_s; a.beta_o = p->beta_o;
    a.F_down = out->F_down; a.nlogpo1 = out->nlogpo1; a.kl_s = out->kl_s; a.kl_s_anal = out->kl_s_anal;
    a.kl_naive = out->kl_naive; a.kl_naive_anal = out->kl_naive_anal;
    return a;
}

}  // namespace host
}  // namespace efe

extern "C" {

// ---- training-side free energy (loss.hip) -------------------------------------------------------------
int efe_free_energy(efe_ctx* ctx, const float* o0, const float* o1, const float* pi0, const float* log_Ppi, int M, const efe_fe_params* params,
                    const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!o0 || !o1 || !pi0 || !log_Ppi || !nz || !out || M < 1)
        return ctx->fail("efe_free_energy: bad arguments (o0, o1, pi0, log_Ppi, params, nz and out must be non-NULL, M >= 1)");
    if (fe_params(ctx, params, true, "efe_free_energy")) return 1;
    if (!out->F_top || !out->F_mid || !out->F_down) return ctx->fail("efe_free_energy: out->F_top, out->F_mid and out->F_down are required");
    const int A = ctx->pi_dim;
    const uint64_t seed = nz->seed;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), stage = nz->stage, ro = nz->row_offset;
    float* enc0 = ctx->allocT<float>((size_t)M * 32);
    float* enc1 = ctx->allocT<float>((size_t)M * 32);
    float* enc2 = ctx->allocT<float>((size_t)M * 32);
    float* tr = ctx->allocT<float>((size_t)M * 32);
    float* l32 = ctx->allocT<float>((size_t)M * 32);
    float* x16 = ctx->allocT<float>((size_t)M * 16);
    float* xm = ctx->allocT<float>((size_t)M * 16);
    float* dec_in = ctx->allocT<float>((size_t)M * 16);
    float* s0 = out->s0 ? out->s0 : ctx->allocT<float>((size_t)M * S_DIM);
    float* q = out->Qpi ? out->Qpi : ctx->allocT<float>((size_t)M * A);
    float* logq = ctx->allocT<float>((size_t)M * A);
    float* omega = out->omega ? out->omega : ctx->allocT<float>((size_t)M);
    const float* o0c = fe_obs(ctx, o0, M, st);
    const float* o1c = fe_obs(ctx, o1, M, st);
    if (!enc0 || !enc1 || !enc2 || !tr || !l32 || !x16 || !xm || !dec_in || !s0 || !q || !logq || !omega || !o0c || !o1c) return 1;
    const float* eps_q0 = eps;
    const float* eps_t = eps ? eps + (size_t)M * S_DIM : nullptr;
    const float* eps_d = eps ? eps + (size_t)2 * M * S_DIM : nullptr;
    // s0 = encoder_with_sample(o0): pass FE_Q0; the habit head reads [s0 | 0] (root_post with pi_dim 0)
    if (run_encoder(ctx, o0c, M, pass_noise(nz, PASS_FE_Q0, 0, M), enc0, st)) return 1;
    launch_root_post(enc0, nullptr, eps_q0, x16, s0, M, 0, k0, k1, PASS_FE_Q0, 0, stage, ro, 0, st);
    if (run_habit(ctx, x16, M, l32, st)) return 1;
    launch_softmax4(l32, nullptr, q, logq, M, A, st);
    // qs1_mean, qs1_logvar = encoder(o1): pass FE_Q1
    if (run_encoder(ctx, o1c, M, pass_noise(nz, PASS_FE_Q1, 0, M), enc1, st)) return 1;
    if (out->qs1_mean || out->qs1_logvar) launch_split_enc(enc1, out->qs1_mean, out->qs1_logvar, M, st);
    // ps1 = transition_with_sample(pi0, s0): pass FE_T
    launch_pack_x(pi0, s0, xm, M, A, S_DIM, st);
    if (run_mid(ctx, xm, 0, M, tr, pass_noise(nz, PASS_FE_T, 0, M), st)) return 1;
    if (out->ps1_mean || out->ps1_logvar) launch_split_enc(tr, out->ps1_mean, out->ps1_logvar, M, st);
    if (out->ps1) launch_root_post(tr, nullptr, eps_t, nullptr, out->ps1, M, 0, k0, k1, PASS_FE_T, 0, stage, ro, A, st);
    {   // F_top, omega, F_mid
        FeArgs a{};
        a.M = M; a.A = A; a.q = q; a.logq = logq; a.log_Ppi = log_Ppi;
        a.kl_pi_anal = out->kl_pi_anal; a.kl_pi = out->kl_pi; a.F_top = out->F_top;
        fe_omega(a, params); a.omega_out = omega;
        a.q1_mean = enc1; a.q1_lv = enc1 + 10; a.q1_ld = 32; a.p1_mean = tr; a.p1_lv = tr + 10; a.p1_ld = 32;
        a.kl_mid_anal = out->kl_s_mid_anal; a.kl_mid = out->kl_s_mid; a.F_mid = out->F_mid;
        launch_fe_top_mid(a, st);
    }
    // compute_loss_down: its own encoder pass over o1 + sample (FE_DOWN), the decoder (FE_DOWN), then k_fe_down
    if (run_encoder(ctx, o1c, M, pass_noise(nz, PASS_FE_DOWN, 0, M), enc2, st)) return 1;
    launch_root_post(enc2, nullptr, eps_d, dec_in, out->qs1, M, 0, k0, k1, PASS_FE_DOWN, 0, stage, ro, 0, st);
    const FeArgs d = fe_down_args(ctx, M, o1, enc2, tr, tr + 10, 32, params, omega, out);
    if (fe_down(ctx, dec_in, M, pass_noise(nz, PASS_FE_DOWN, 0, M), d, out->po1, st)) return 1;
    return call.finish();
}

int efe_loss_top(efe_ctx* ctx, const float* s, const float* log_Ppi, int M, efe_fe_out* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s || !log_Ppi || !out || M < 1) return ctx->fail("efe_loss_top: bad arguments (s, log_Ppi and out must be non-NULL, M >= 1)");
    if (!out->F_top) return ctx->fail("efe_loss_top: out->F_top is required");
    const int A = ctx->pi_dim;
    float* x16 = ctx->allocT<float>((size_t)M * 16);
    float* l32 = ctx->allocT<float>((size_t)M * 32);
    float* q = out->Qpi ? out->Qpi : ctx->allocT<float>((size_t)M * A);
    float* logq = ctx->allocT<float>((size_t)M * A);
    if (!x16 || !l32 || !q || !logq) return 1;
    launch_pad16(s, x16, M, S_DIM, st);
    if (run_habit(ctx, x16, M, l32, st)) return 1;
    launch_softmax4(l32, nullptr, q, logq, M, A, st);
    FeArgs a{};
    a.M = M; a.A = A; a.q = q; a.logq = logq; a.log_Ppi = log_Ppi;
    a.kl_pi_anal = out->kl_pi_anal; a.kl_pi = out->kl_pi; a.F_top = out->F_top;
    a.omega_mode = 1; a.omega_scalar = 1.0f;           // (no mid part: omega unused)
    launch_fe_top_mid(a, st);
    return call.finish();
}

int efe_loss_mid(efe_ctx* ctx, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M,
                 const efe_fe_params* params, const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s0 || !pi0 || !qs1_mean || !qs1_logvar || !nz || !out || M < 1)
        return ctx->fail("efe_loss_mid: bad arguments (s0, pi0, qs1_mean, qs1_logvar, params, nz and out must be non-NULL, M >= 1)");
    if (fe_params(ctx, params, false, "efe_loss_mid")) return 1;
    if (!out->F_mid) return ctx->fail("efe_loss_mid: out->F_mid is required");
    float* xm = ctx->allocT<float>((size_t)M * 16);
    float* tr = ctx->allocT<float>((size_t)M * 32);
    if (!xm || !tr) return 1;
    launch_pack_x(pi0, s0, xm, M, ctx->pi_dim, S_DIM, st);
    const NoiseCfg nc = pass_noise(nz, nz->pass, nz->sample, M);
    if (run_mid(ctx, xm, 0, M, tr, nc, st)) return 1;
    if (out->ps1_mean || out->ps1_logvar) launch_split_enc(tr, out->ps1_mean, out->ps1_logvar, M, st);
    if (out->ps1) launch_root_post(tr, nullptr, eps, nullptr, out->ps1, M, 0, nc.k0, nc.k1, nz->pass, nz->sample, nz->stage, nz->row_offset, ctx->pi_dim, st);
    FeArgs a{};
    a.M = M; a.A = ctx->pi_dim;
    fe_omega(a, params); a.omega_out = nullptr;
    a.q1_mean = qs1_mean; a.q1_lv = qs1_logvar; a.q1_ld = S_DIM; a.p1_mean = tr; a.p1_lv = tr + 10; a.p1_ld = 32;
    a.kl_mid_anal = out->kl_s_mid_anal; a.kl_mid = out->kl_s_mid; a.F_mid = out->F_mid;
    launch_fe_top_mid(a, st);
    return call.finish();
}

int efe_loss_down(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!o1 || !ps1_mean || !ps1_logvar || !nz || !out || M < 1)
        return ctx->fail("efe_loss_down: bad arguments (o1, ps1_mean, ps1_logvar, params, nz and out must be non-NULL, M >= 1)");
    if (fe_params(ctx, params, false, "efe_loss_down")) return 1;
    if (!out->F_down) return ctx->fail("efe_loss_down: out->F_down is required");
    float* enc = ctx->allocT<float>((size_t)M * 32);
    float* dec_in = ctx->allocT<float>((size_t)M * 16);
    const float* o1c = fe_obs(ctx, o1, M, st);
    if (!enc || !dec_in || !o1c) return 1;
    const NoiseCfg nc = pass_noise(nz, nz->pass, nz->sample, M);
    if (run_encoder(ctx, o1c, M, nc, enc, st)) return 1;
    if (out->qs1_mean || out->qs1_logvar) launch_split_enc(enc, out->qs1_mean, out->qs1_logvar, M, st);
    launch_root_post(enc, nullptr, eps, dec_in, out->qs1, M, 0, nc.k0, nc.k1, nz->pass, nz->sample, nz->stage, nz->row_offset, 0, st);
    const FeArgs d = fe_down_args(ctx, M, o1, enc, ps1_mean, ps1_logvar, S_DIM, params,
                                  params->omega_mode == EFE_OMEGA_ARRAY ? params->omega : nullptr, out);
    if (fe_down(ctx, dec_in, M, nc, d, out->po1, st)) return 1;
    return call.finish();
}

// ---- the epoch report (eval.hip) ----------------------------------------------------------------------
// Reads the caller's arrays and writes the caller's row: no scratch, no weights, so the scope is Mode::device.  Every refusal comes before
// the launch.
int efe_eval_stats(efe_ctx* ctx, const efe_eval_in* in, int M, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::device, st); if (!call) return call.refused("efe_eval_stats");
    if (!in || !out) return ctx->fail("efe_eval_stats: in and out must be non-NULL");
    if (M < 1) return ctx->fail("efe_eval_stats: M must be >= 1");
    if (M > EFE_EVAL_MAX_ROWS) return ctx->fail("efe_eval_stats: M = " + std::to_string(M) + " is above the cap of " + std::to_string((int)EFE_EVAL_MAX_ROWS) + " rows");
    const float* fe[10] = {in->F_top, in->F_mid, in->F_down, in->nlogpo1, in->kl_s, in->kl_naive, in->kl_pi, in->kl_s_anal, in->kl_naive_anal, in->kl_pi_anal};
    int n_fe = 0;
    for (const float* p : fe) n_fe += p ? 1 : 0;
    if (n_fe != 0 && n_fe != 10)
        return ctx->fail("efe_eval_stats: partial FE group (" + std::to_string(n_fe) + " of its 10 arrays given: F_top, F_mid, F_down, nlogpo1, kl_s, kl_naive, kl_pi, kl_s_anal, kl_naive_anal, kl_pi_anal)");
    if (!in->s0 != !in->S_real) return ctx->fail("efe_eval_stats: partial RHO group (s0 and S_real go together)");
    const bool r_any = in->o1_r || in->po1_r;
    if (r_any && (!in->o1_r || !in->po1_r || in->Mr < 1)) return ctx->fail("efe_eval_stats: partial R group (o1_r, po1_r and Mr >= 1 go together)");
    if (r_any && in->Mr > EFE_EVAL_MAX_ROWS) return ctx->fail("efe_eval_stats: Mr = " + std::to_string(in->Mr) + " is above the cap of " + std::to_string((int)EFE_EVAL_MAX_ROWS) + " rows");
    if (!n_fe && !in->qs1 && !in->s0 && !r_any) return ctx->fail("efe_eval_stats: no input group (FE, TC, RHO or R) given");
    if (n_fe && ctx->pi_dim != 4) return ctx->fail("efe_eval_stats: the row layout holds kl_div_pi_anal [4], this context has pi_dim " + std::to_string(ctx->pi_dim));
    if (r_any && (ctx->chan != 1 || ctx->res != 64)) return ctx->fail("efe_eval_stats: mse_r reads 1 x 64 x 64 images");
    EvalArgs a{};
    for (int k = 0; k < 7; ++k) a.row[k] = fe[k];
    a.kl_s_anal = in->kl_s_anal; a.kl_naive_anal = in->kl_naive_anal; a.kl_pi_anal = in->kl_pi_anal;
    a.qs1 = in->qs1; a.s0 = in->s0; a.S_real = in->S_real; a.o1_r = in->o1_r; a.po1_r = in->po1_r;
    a.M = M; a.Mr = r_any ? in->Mr : 0; a.A = ctx->pi_dim; a.out = out;
    launch_eval_stats(a, st);
    return call.finish();
}

// The mutual-information table (eval_mi.hip).  It reads the caller's arrays and no weights, and keeps its 32 column statistics and its
// per-slice partial sums in ctx->mi_ws, so the scope is Mode::ordered: a call on another stream waits for the previous one.  Every refusal
// comes before the launch.
int efe_eval_mi(efe_ctx* ctx, const efe_eval_mi_in* in, int M, float* out, int32_t* counts, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::ordered, st); if (!call) return call.refused("efe_eval_mi");
    if (!in || !out) return ctx->fail("efe_eval_mi: in and out must be non-NULL");
    if (!in->s0 || !in->S_real) return ctx->fail("efe_eval_mi: in->s0 and in->S_real must be non-NULL");
    if (in->n_neighbors < 1 || in->n_neighbors > EFE_EVAL_MI_MAX_NEIGHBORS)
        return ctx->fail("efe_eval_mi: n_neighbors = " + std::to_string(in->n_neighbors) + " is outside 1 .. " + std::to_string((int)EFE_EVAL_MI_MAX_NEIGHBORS));
    if (M < in->n_neighbors + 1)
        return ctx->fail("efe_eval_mi: M = " + std::to_string(M) + " rows hold no " + std::to_string(in->n_neighbors) + " neighbours of a point (M must be >= n_neighbors + 1)");
    if (M > EFE_EVAL_MAX_ROWS) return ctx->fail("efe_eval_mi: M = " + std::to_string(M) + " is above the cap of " + std::to_string((int)EFE_EVAL_MAX_ROWS) + " rows");
    EvalMiArgs a{};
    a.s0 = in->s0; a.S_real = in->S_real; a.noise = in->noise; a.M = M; a.k = in->n_neighbors;
    a.k0 = (uint32_t)in->seed; a.k1 = (uint32_t)(in->seed >> 32); a.stage = in->stage;
    a.ws = ctx->mi_ws; a.psi = ctx->mi_ws + EVAL_MI_WS; a.out = out; a.counts = counts;
    launch_eval_mi(a, st);
    return call.finish();
}

}  // extern "C"
