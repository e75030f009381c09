// Host side of the engine, training: the gradients of the habit net, the transition net and ModelDown (train*.hip), their optimiser
// steps, and one whole training step (efe_train_step).  Each `*_run` helper is an entry point's body inside its call scope, shared
// with efe_train_step.
#include "engine.h"

namespace {

// "top" = ModelTop.qpi_net, "ps_net" = ModelMid.ps_net (the reference's module name; "mid" stays refused: a test of the habit-net
// commit pins it as an unknown part)
TrainPart* train_part(efe_ctx* ctx, const char* part, const char* who) {
    if (part && !strcmp(part, "top")) return &ctx->top_train;
    if (part && !strcmp(part, "ps_net")) return &ctx->mid_train;
    ctx->fail(std::string(who) + ": part must be \"top\" (habit net) or \"ps_net\" (transition net), the trainable parts");
    return nullptr;
}
// (tp == nullptr: the scalars alone, for ModelDown's step, which has no layer table)
int adam_args(efe_ctx* ctx, const TrainPart* tp, const efe_adam_params* hp, AdamArgs& a, const char* who) {
    if (!hp || hp->step < 1 || !(hp->lr >= 0.0) || !(hp->beta1 >= 0.0 && hp->beta1 < 1.0) || !(hp->beta2 >= 0.0 && hp->beta2 < 1.0) || !(hp->eps >= 0.0))
        return ctx->fail(std::string(who) + ": bad hyper-parameters (step >= 1, lr >= 0, 0 <= beta < 1, eps >= 0)");
    // torch.optim.Adam's scalars, in double as Python computes them, rounded once
    const double bc1 = 1.0 - std::pow(hp->beta1, (double)hp->step), bc2 = 1.0 - std::pow(hp->beta2, (double)hp->step);
    a.net = tp ? tp->net_dev : nullptr;
    a.omb1 = (float)(1.0 - hp->beta1); a.b2 = (float)hp->beta2; a.omb2 = (float)(1.0 - hp->beta2);
    a.bc2_sqrt = (float)std::sqrt(bc2); a.step_size = (float)(hp->lr / bc1); a.eps = (float)hp->eps;
    return 0;
}
// the Philox fields of a training call; row = the first row of the call's row group
TrainKey train_key(const efe_noise* nz, uint32_t row = 0) {
    return TrainKey{(uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), nz->row_offset + row, stream_id(nz->pass, nz->sample), nz->stage};
}
// the arguments of k_mid_grad after efe_loss_mid's checks (params: omega per row or scalar; nz: the keys of every dropout mask)
// (arrays_ok: the entry point's own arrays -- the gradient, or both moments -- are non-NULL)
int mid_grad_args(efe_ctx* ctx, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, bool arrays_ok, MidGradArgs& a, const char* who) {
    if (!s0 || !pi0 || !qs1_mean || !qs1_logvar || !nz || !arrays_ok || M < 1)
        return ctx->fail(std::string(who) + ": bad arguments (s0, pi0, qs1_mean, qs1_logvar, params, nz and the gradient / state arrays must be non-NULL, M >= 1)");
    if (fe_params(ctx, params, false, who)) return 1;
    a.net = ctx->mid_train.net_dev;
    a.s0 = s0; a.pi0 = pi0; a.q1_mean = qs1_mean; a.q1_lv = qs1_logvar;
    a.omega_mode = params->omega_mode; a.omega_in = params->omega; a.omega_scalar = params->omega_scalar;
    // (the kernel writes all three: scratch stands in for an output the caller does not want)
    a.p1_mean = ps1_mean ? ps1_mean : ctx->allocT<float>((size_t)M * S_DIM);
    a.p1_lv = ps1_logvar ? ps1_logvar : ctx->allocT<float>((size_t)M * S_DIM);
    a.F_mid = F_mid ? F_mid : ctx->allocT<float>((size_t)M);
    if (!a.p1_mean || !a.p1_lv || !a.F_mid) return 1;
    a.M = M; a.A = ctx->pi_dim; a.S = S_DIM; a.inv_M = 1.0f / (float)M;
    a.key = train_key(nz);
    return 0;
}
// the tail of a gradient call (adam == nullptr) or of a training step over G partial-gradient slabs: launch(slabs) runs the backward
// kernel; then the slabs are summed into `grad` (G == 1: the one slab IS grad), or k_adam forms the gradient by the same ascending sum
template <class Launch>
int grad_or_step(efe_ctx* ctx, TrainPart& tp, int G, float* grad, AdamArgs* adam, hipStream_t st, Launch launch) {
    const int P = tp.net.P;
    float* slabs = (!adam && G == 1) ? grad : ctx->allocT<float>((size_t)G * P);
    if (!slabs) return 1;
    launch(slabs);
    if (adam) {
        adam->g = slabs; adam->nslab = G;
        tp.dirty = true;
        launch_adam(*adam, P, st);
    } else if (G > 1) launch_slab_sum(slabs, G, P, grad, st);
    return 0;
}

// efe_train_top inside its call scope, for efe_train_step too (`who` names the entry point in the messages).  Every refusal comes before the launch.
int train_top_run(efe_ctx* ctx, const char* who, const float* s, const float* log_Ppi, int M, float* kl_pi, float* exp_avg, float* exp_avg_sq,
                  const efe_adam_params* hp, hipStream_t st) {
    if (!s || !log_Ppi || !exp_avg || !exp_avg_sq || M < 1)
        return ctx->fail(std::string(who) + ": bad arguments (s, log_Ppi, exp_avg and exp_avg_sq must be non-NULL, M >= 1)");
    TrainPart& tp = ctx->top_train;
    AdamArgs a{};
    if (adam_args(ctx, &tp, hp, a, who)) return 1;
    a.m = exp_avg; a.v = exp_avg_sq;
    return grad_or_step(ctx, tp, train_slabs(M), nullptr, &a, st, [&](float* slabs) {
        launch_top_grad(TopGradArgs{tp.net_dev, s, log_Ppi, kl_pi, slabs, M, ctx->pi_dim, 1.0f / (float)M}, st); });
}

// efe_train_mid inside its call scope, for efe_train_step too.  Every refusal comes before the launch.
int train_mid_run(efe_ctx* ctx, const char* who, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M,
                  const efe_fe_params* params, const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* exp_avg, float* exp_avg_sq,
                  const efe_adam_params* hp, hipStream_t st) {
    MidGradArgs g{};
    if (mid_grad_args(ctx, s0, pi0, qs1_mean, qs1_logvar, M, params, nz, ps1_mean, ps1_logvar, F_mid, exp_avg && exp_avg_sq, g, who)) return 1;
    TrainPart& tp = ctx->mid_train;
    AdamArgs a{};
    if (adam_args(ctx, &tp, hp, a, who)) return 1;
    a.m = exp_avg; a.v = exp_avg_sq;
    return grad_or_step(ctx, tp, train_mid_slabs(M), nullptr, &a, st, [&](float* slabs) { g.slabs = slabs; launch_mid_grad(g, st); });
}

// the dense head's side of the call: its input, the keys of its four dropout masks, its outputs (all nullable but s and nz)
struct DecHeadIO { const float* s; const efe_noise* nz; float* d_s; float *h1, *h2, *h3, *h4; };

// what every decoder-gradient call refuses, in this order and before its first launch: M, the required pointers, the geometry, the
// split-operand options, the scale (negative = beta_o / M, written back)
int dec_grad_checks(efe_ctx* ctx, const char* who, int M, bool ptrs, const char* ptr_msg, bool geometry, float& scale, float beta_o) {
    const std::string w(who);
    if (M <= 0) return ctx->fail(w + ": M must be >= 1");
    if (!ptrs) return ctx->fail(w + ptr_msg);
    if (!geometry) return ctx->fail(w + ": built for the 1 x 64 x 64 geometry only");
    if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
    if (!(scale >= 0.0f)) {
        if (!(scale < 0.0f) || !std::isfinite(beta_o)) return ctx->fail(w + ": scale is NaN, or negative (= beta_o / M) with a non-finite beta_o");
        scale = beta_o / (float)M;
    }
    return 0;
}

// The decoder's gradient as the row groups of one call: open() checks the arguments and takes the scratch, group(m0) queues the forward and
// backward of rows [m0, m0 + rows(m0)), close() joins the slabs.  efe_dec_tail_grad, efe_dec_grad and efe_down_grad (which runs the
// encoder's group around each of the decoder's) share it.
// hd == nullptr: the tail alone, from the caller's h4 to the caller's d_h4 (nullable), grad [DEC_TAIL_P]; else grad [DEC_P] and h4 / d_h4 unused
struct DecGrad {
    efe_ctx* ctx; const DecHeadIO* hd; const float* h4; float* d_h4; const float* o1; int M; float scale;
    float *nlogpo1, *po1, *grad, *y1, *y2, *y3;
    hipStream_t st;
    DecTailPlan p; DecHeadPlan hp{};
    float *s1, *s2, *s3, *sp, *g4, *g3, *g2, *g1, *tgrad, *tslabs;
    float *a1 = nullptr, *a2 = nullptr, *a3 = nullptr, *a4 = nullptr, *dh4 = nullptr, *part = nullptr, *hslabs = nullptr;
    int open(efe_ctx* ctx_, const char* who, const DecHeadIO* hd_, const float* h4_, float* d_h4_, const float* o1_, int M_, float scale_, float beta_o,
             float* nlogpo1_, float* po1_, float* grad_, float* y1_, float* y2_, float* y3_, hipStream_t st_);
    int rows(int m0) const { return std::min(p.C, M - m0); }
    const float* po_of(int m0) const { return po1 ? po1 + (size_t)m0 * 4096 : sp; }      // the images of the group that starts at row m0
    void group(int m0);
    void close();
};
int DecGrad::open(efe_ctx* ctx_, const char* who, const DecHeadIO* hd_, const float* h4_, float* d_h4_, const float* o1_, int M_, float scale_, float beta_o,
                  float* nlogpo1_, float* po1_, float* grad_, float* y1_, float* y2_, float* y3_, hipStream_t st_) {
    ctx = ctx_; hd = hd_; h4 = h4_; d_h4 = d_h4_; o1 = o1_; M = M_; scale = scale_;
    nlogpo1 = nlogpo1_; po1 = po1_; grad = grad_; y1 = y1_; y2 = y2_; y3 = y3_; st = st_;
    const bool ptrs = (hd ? hd->s && hd->nz : h4 != nullptr) && o1 && nlogpo1 && grad;
    if (dec_grad_checks(ctx, who, M, ptrs, hd ? ": s, o1, nz, nlogpo1 and grad must be non-NULL" : ": h4, o1, nlogpo1 and grad must be non-NULL",
                        ctx->chan == 1 && ctx->res == 64 && (hd ? ctx->dec_raw : ctx->dect_raw), scale, beta_o)) return 1;
    p = dec_tail_plan(M, !y1, !y2, !y3, !po1);
    s1 = ctx->allocT<float>(p.y1); s2 = ctx->allocT<float>(p.y2); s3 = ctx->allocT<float>(p.y3); sp = ctx->allocT<float>(p.po);
    g4 = ctx->allocT<float>(p.g4); g3 = ctx->allocT<float>(p.g3); g2 = ctx->allocT<float>(p.g2); g1 = ctx->allocT<float>(p.g1);
    tgrad = hd ? grad + DEC_HEAD_P : grad;           // the tail's gradient
    tslabs = p.G > 1 ? ctx->allocT<float>(p.slabs) : tgrad;
    if (!s1 || !s2 || !s3 || !sp || !g4 || !g3 || !g2 || !g1 || !tslabs) return 1;
    if (hd) {
        hp = dec_head_plan(M, !hd->h1, !hd->h2, !hd->h3, !hd->h4);
        a1 = ctx->allocT<float>(hp.h1); a2 = ctx->allocT<float>(hp.h2); a3 = ctx->allocT<float>(hp.h3); a4 = ctx->allocT<float>(hp.h4);
        dh4 = ctx->allocT<float>(hp.dh4); part = ctx->allocT<float>(hp.part);
        hslabs = hp.G > 1 ? ctx->allocT<float>(hp.slabs) : grad;
        if (!a1 || !a2 || !a3 || !a4 || !dh4 || !part || !hslabs) return 1;
    }
    return 0;
}
// one row group: boundaries at multiples of DEC_TAIL_ROWS, a function of M alone
void DecGrad::group(int m0) {
    {
        const int rows = this->rows(m0);
        DecHeadArgs h{};
        if (hd) {
            h.w = ctx->dec_raw; h.s = hd->s + (size_t)m0 * S_DIM;
            h.h1 = hd->h1 ? hd->h1 + (size_t)m0 * 256 : a1; h.h2 = hd->h2 ? hd->h2 + (size_t)m0 * 256 : a2; h.h3 = hd->h3 ? hd->h3 + (size_t)m0 * 256 : a3;
            h.h4 = hd->h4 ? hd->h4 + (size_t)m0 * DEC_TAIL_Y1 : a4;
            h.g4 = dh4; h.part = part; h.ds = hd->d_s ? hd->d_s + (size_t)m0 * S_DIM : nullptr; h.grad = grad; h.slabs = hslabs;
            h.rows = rows; h.first = m0 == 0; h.key = train_key(hd->nz, (uint32_t)m0);
            launch_dec_head_fwd(h, st);
        }
        DecTailArgs a{};
        a.w = ctx->dect_raw; a.h4 = hd ? h.h4 : h4 + (size_t)m0 * DEC_TAIL_Y1; a.o1 = o1 + (size_t)m0 * 4096;
        a.y1 = y1 ? y1 + (size_t)m0 * DEC_TAIL_Y1 : s1; a.y2 = y2 ? y2 + (size_t)m0 * DEC_TAIL_Y2 : s2; a.y3 = y3 ? y3 + (size_t)m0 * DEC_TAIL_Y3 : s3;
        a.po = po1 ? po1 + (size_t)m0 * 4096 : sp; a.nlogpo1 = nlogpo1 + m0;
        a.g4 = g4; a.g3 = g3; a.g2 = g2; a.g1 = g1; a.dh4 = hd ? dh4 : d_h4 ? d_h4 + (size_t)m0 * DEC_TAIL_Y1 : nullptr;
        a.slabs = tslabs; a.rows = rows; a.G = p.G; a.first = m0 == 0; a.scale = scale;
        launch_dec_tail_group(a, st);
        if (hd) launch_dec_head_bwd(h, st);
    }
}
void DecGrad::close() {
    if (p.G > 1) launch_slab_sum(tslabs, p.G, DEC_TAIL_P, tgrad, st);
    if (hd && hp.G > 1) launch_slab_sum(hslabs, hp.G, DEC_HEAD_SMALL_P, grad, st);
    ctx->last_macs += (int64_t)M * 3 * (38928384 + (hd ? 4328960 : 0));      // forward, data gradient, weight gradient of the four (eight) layers
}
int dec_grad(efe_ctx* ctx, const char* who, const DecHeadIO* hd, const float* h4, float* d_h4, const float* o1, int M, float scale, float beta_o,
             float* nlogpo1, float* po1, float* grad, float* y1, float* y2, float* y3, hipStream_t st) {
    DecGrad d;
    if (d.open(ctx, who, hd, h4, d_h4, o1, M, scale, beta_o, nlogpo1, po1, grad, y1, y2, y3, st)) return 1;
    for (int m0 = 0; m0 < M; m0 += d.p.C) d.group(m0);
    d.close();
    return 0;
}

// efe_dec_tail_grad_g and efe_dec_grad_g inside their call scope, as the row groups of one call (open / group / close, so that efe_down_grad_g
// can run the encoder's group around each of the decoder's): the decoder's gradient by the run-time-geometry kernels (train_dec_g.hip,
// train_dec_head_g.hip), at every admitted geometry.  Row groups of geo.rows_per_pass() rows; scratch of one group from the arena: the
// activations the caller gives no output for, the four gradients, and G slabs (none at G = 1: the gradient itself).
// hd == nullptr: the tail alone, from the caller's h4 to the caller's d_h4 (nullable), grad [geo.P()].  Else the whole decoder, grad
// [hg.P() + geo.P()], h4 / d_h4 unused: per group the head's forward, launch_dec_tail_g_group exactly as without the head (on the group's h4,
// d_h4 to scratch), the head's backward; the head takes h1..h4 and d_h4 of one group and the S x rows x 256 partials of d_h3 as well.
struct DecGradG {
    efe_ctx* ctx; const DecHeadIO* hd; const float* h4; const float* o1; int M; float scale;
    float *nlogpo1, *po1, *d_h4, *grad, *y1, *y2, *y3;
    hipStream_t st;
    DecTailGeo geo; DecHeadGeo hg;
    int C, G, GH, P;
    float *tgrad, *s1, *s2, *s3, *sp, *g4, *g3, *g2, *g1, *slabs;
    float *a1 = nullptr, *a2 = nullptr, *a3 = nullptr, *a4 = nullptr, *dh4 = nullptr, *part = nullptr, *hslabs = nullptr;
    int open(efe_ctx* ctx_, const char* who, const DecHeadIO* hd_, const float* h4_, const float* o1_, int M_, float scale_, float beta_o, float* nlogpo1_,
             float* po1_, float* d_h4_, float* grad_, float* y1_, float* y2_, float* y3_, hipStream_t st_) {
        ctx = ctx_; hd = hd_; h4 = h4_; o1 = o1_; M = M_; scale = scale_; nlogpo1 = nlogpo1_; po1 = po1_; d_h4 = d_h4_; grad = grad_;
        y1 = y1_; y2 = y2_; y3 = y3_; st = st_;
        // (a context without the raw copy cannot exist once committed: the geometry test of the shared checks stands for "the copy is there")
        const bool ptrs = (hd ? hd->s && hd->nz : h4 != nullptr) && o1 && nlogpo1 && grad;
        if (dec_grad_checks(ctx, who, M, ptrs, hd ? ": s, o1, nz, nlogpo1 and grad must be non-NULL" : ": h4, o1, nlogpo1 and grad must be non-NULL",
                            (hd ? ctx->dec_raw_g : ctx->dect_raw_g) != nullptr, scale, beta_o))
            return 1;
        geo = DecTailGeo{ctx->base, ctx->chan, ctx->last_s1 ? 1 : 2};
        hg = DecHeadGeo{ctx->base};
        C = std::min(geo.rows_per_pass(), M); G = dec_tail_slabs(M); P = geo.P();
        const size_t n = (size_t)C;
        tgrad = hd ? grad + hg.P() : grad;        // the tail's gradient
        s1 = y1 ? nullptr : ctx->allocT<float>(n * geo.y1());
        s2 = y2 ? nullptr : ctx->allocT<float>(n * geo.y2());
        s3 = y3 ? nullptr : ctx->allocT<float>(n * geo.y3());
        sp = po1 ? nullptr : ctx->allocT<float>(n * geo.img());
        g4 = ctx->allocT<float>(n * geo.img());
        g3 = ctx->allocT<float>(n * geo.y3());
        g2 = ctx->allocT<float>(n * geo.y2());
        g1 = ctx->allocT<float>(n * geo.y1());
        slabs = G > 1 ? ctx->allocT<float>((size_t)G * P) : tgrad;
        if ((!y1 && !s1) || (!y2 && !s2) || (!y3 && !s3) || (!po1 && !sp) || !g4 || !g3 || !g2 || !g1 || !slabs) return 1;
        GH = dec_head_slabs(M);
        if (hd) {
            if (!hd->h1) a1 = ctx->allocT<float>(n * 256);
            if (!hd->h2) a2 = ctx->allocT<float>(n * 256);
            if (!hd->h3) a3 = ctx->allocT<float>(n * 256);
            if (!hd->h4) a4 = ctx->allocT<float>(n * geo.y1());
            dh4 = ctx->allocT<float>(n * geo.y1());
            part = ctx->allocT<float>((size_t)hg.segs() * n * 256);
            hslabs = GH > 1 ? ctx->allocT<float>((size_t)GH * DEC_HEAD_SMALL_P) : grad;
            if ((!hd->h1 && !a1) || (!hd->h2 && !a2) || (!hd->h3 && !a3) || (!hd->h4 && !a4) || !dh4 || !part || !hslabs) return 1;
        }
        return 0;
    }
    int rows(int m0) const { return std::min(C, M - m0); }
    const float* po_of(int m0) const { return po1 ? po1 + (size_t)m0 * geo.img() : sp; }      // the images (NCHW) of the group that starts at row m0
    void group(int m0) {
        const size_t m = (size_t)m0;
        const int rows = this->rows(m0);
        DecHeadGArgs h{};
        if (hd) {
            h.geo = hg; h.w = ctx->dec_raw_g; h.s = hd->s + m * S_DIM;
            h.h1 = hd->h1 ? hd->h1 + m * 256 : a1; h.h2 = hd->h2 ? hd->h2 + m * 256 : a2; h.h3 = hd->h3 ? hd->h3 + m * 256 : a3;
            h.h4 = hd->h4 ? hd->h4 + m * geo.y1() : a4;
            h.g4 = dh4; h.part = part; h.ds = hd->d_s ? hd->d_s + m * S_DIM : nullptr; h.grad = grad; h.slabs = hslabs;
            h.rows = rows; h.first = m0 == 0; h.tile0 = m0 / 16; h.key = train_key(hd->nz, (uint32_t)m0);
            launch_dec_head_g_fwd(h, st);
        }
        DecTailGArgs a{};
        a.geo = geo; a.w = ctx->dect_raw_g; a.h4 = hd ? h.h4 : h4 + m * geo.y1(); a.o1 = o1 + m * geo.img();
        a.y1 = y1 ? y1 + m * geo.y1() : s1; a.y2 = y2 ? y2 + m * geo.y2() : s2; a.y3 = y3 ? y3 + m * geo.y3() : s3;
        a.po = po1 ? po1 + m * geo.img() : sp; a.nlogpo1 = nlogpo1 + m0;
        a.g4 = g4; a.g3 = g3; a.g2 = g2; a.g1 = g1; a.dh4 = hd ? dh4 : d_h4 ? d_h4 + m * geo.y1() : nullptr;
        a.slabs = slabs; a.rows = rows; a.G = G; a.first = m0 == 0; a.scale = scale;
        launch_dec_tail_g_group(a, st);
        if (hd) launch_dec_head_g_bwd(h, st);
    }
    void close() {
        if (G > 1) launch_slab_sum(slabs, G, P, tgrad, st);
        if (hd && GH > 1) launch_slab_sum(hslabs, GH, DEC_HEAD_SMALL_P, grad, st);
        // forward, data gradient, weight gradient of the four layers: 2 x 36 864 B^2, 18 432 (2B)^2, 288 C R^2 multiply-adds each; of the head's
        // four: 10 x 256, 2 x 256 x 256, 256 F
        const int64_t BB = (int64_t)geo.B * geo.B, RR = (int64_t)geo.R() * geo.R();
        ctx->last_macs += (int64_t)M * 3 * (2 * 36864 * BB + 18432 * 4 * BB + 288 * geo.C * RR);
        if (hd) ctx->last_macs += (int64_t)M * 3 * (2560 + 131072 + 256 * (int64_t)hg.F());
    }
};
int dec_grad_g_run(efe_ctx* ctx, const char* who, const DecHeadIO* hd, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1,
                   float* po1, float* d_h4, float* grad, float* y1, float* y2, float* y3, hipStream_t st) {
    DecGradG d;
    if (d.open(ctx, who, hd, h4, o1, M, scale, beta_o, nlogpo1, po1, d_h4, grad, y1, y2, y3, st)) return 1;
    for (int m0 = 0; m0 < M; m0 += d.C) d.group(m0);
    d.close();
    return 0;
}

// ---- the encoder's training forward and backward (train_enc.hip) as the row groups of one call, the same way ---------------------------
// the encoder's stored activations of one row group (those the caller gives no output for), the gradients at the four convolutions'
// outputs, and the two sets of slabs (none at G = 1: the gradient itself)
struct EncGradPlan { int C, GC, GH; size_t y1, y2, y3, y4, h1, h2, h3, g4, g3, g2, g1, cslabs, hslabs; };
EncGradPlan enc_grad_plan(int64_t M, bool own_y1, bool own_y2, bool own_y3, bool own_y4, bool own_h1, bool own_h2, bool own_h3) {
    const size_t C = (size_t)std::min<int64_t>(DEC_TAIL_ROWS, M);
    const int GC = enc_conv_slabs((int)std::min<int64_t>(M, ENC_CONV_SLABS)), GH = enc_head_slabs((int)std::min<int64_t>(M, 16 * ENC_HEAD_SLABS));
    return {(int)C, GC, GH, own_y1 ? C * ENC_Y1 : 0, own_y2 ? C * ENC_Y2 : 0, own_y3 ? C * ENC_Y3 : 0, own_y4 ? C * ENC_Y4 : 0,
            own_h1 ? C * 256 : 0, own_h2 ? C * 256 : 0, own_h3 ? C * 256 : 0, C * ENC_Y4, C * ENC_Y3, C * ENC_Y2, C * ENC_Y1,
            GC > 1 ? (size_t)GC * ENC_CONV_P : 0, GH > 1 ? (size_t)GH * ENC_HEAD_P : 0};
}
struct EncGrad {
    efe_ctx* ctx; const float* o; const float *g_mean, *g_logvar; int M; const efe_noise* nz;
    float *mean, *logvar, *grad, *y1, *y2, *y3, *y4, *h1, *h2, *h3;      // mean / logvar [M][10] are never scratch of one group: the caller's, or whole
    hipStream_t st;
    EncGradPlan p;
    float *s1, *s2, *s3, *s4, *a1, *a2, *a3, *g4, *g3, *g2, *g1, *cslabs, *hslabs;
    // g_mean / g_logvar may be given later (set them before the first bwd()): the composed call forms them per group
    int open(efe_ctx* ctx_, const char* who, const float* o_, int M_, const efe_noise* nz_, float* mean_, float* logvar_, float* grad_,
             float* y1_, float* y2_, float* y3_, float* y4_, float* h1_, float* h2_, float* h3_, hipStream_t st_) {
        ctx = ctx_; o = o_; M = M_; nz = nz_; mean = mean_; logvar = logvar_; grad = grad_;
        y1 = y1_; y2 = y2_; y3 = y3_; y4 = y4_; h1 = h1_; h2 = h2_; h3 = h3_; st = st_; g_mean = g_logvar = nullptr;
        const std::string w(who);
        if (ctx->chan != 1 || ctx->res != 64 || !ctx->enc_raw) return ctx->fail(w + ": built for the 1 x 64 x 64 geometry only");
        if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
        p = enc_grad_plan(M, !y1, !y2, !y3, !y4, !h1, !h2, !h3);
        s1 = ctx->allocT<float>(p.y1); s2 = ctx->allocT<float>(p.y2); s3 = ctx->allocT<float>(p.y3); s4 = ctx->allocT<float>(p.y4);
        a1 = ctx->allocT<float>(p.h1); a2 = ctx->allocT<float>(p.h2); a3 = ctx->allocT<float>(p.h3);
        g4 = ctx->allocT<float>(p.g4); g3 = ctx->allocT<float>(p.g3); g2 = ctx->allocT<float>(p.g2); g1 = ctx->allocT<float>(p.g1);
        if (!mean) mean = ctx->allocT<float>((size_t)M * S_DIM);
        if (!logvar) logvar = ctx->allocT<float>((size_t)M * S_DIM);
        cslabs = p.GC > 1 ? ctx->allocT<float>(p.cslabs) : grad;
        hslabs = p.GH > 1 ? ctx->allocT<float>(p.hslabs) : grad + ENC_CONV_P;
        if (!s1 || !s2 || !s3 || !s4 || !a1 || !a2 || !a3 || !g4 || !g3 || !g2 || !g1 || !mean || !logvar || !cslabs || !hslabs) return 1;
        return 0;
    }
    EncTrainArgs args(int m0) const {
        EncTrainArgs a{};
        a.w = ctx->enc_raw; a.o = o + (size_t)m0 * 4096;
        a.y1 = y1 ? y1 + (size_t)m0 * ENC_Y1 : s1; a.y2 = y2 ? y2 + (size_t)m0 * ENC_Y2 : s2; a.y3 = y3 ? y3 + (size_t)m0 * ENC_Y3 : s3;
        a.y4 = y4 ? y4 + (size_t)m0 * ENC_Y4 : s4;
        a.h1 = h1 ? h1 + (size_t)m0 * 256 : a1; a.h2 = h2 ? h2 + (size_t)m0 * 256 : a2; a.h3 = h3 ? h3 + (size_t)m0 * 256 : a3;
        a.mean = mean + (size_t)m0 * S_DIM; a.logvar = logvar + (size_t)m0 * S_DIM;
        a.g_mean = g_mean ? g_mean + (size_t)m0 * S_DIM : nullptr; a.g_logvar = g_logvar ? g_logvar + (size_t)m0 * S_DIM : nullptr;
        a.g4 = g4; a.g3 = g3; a.g2 = g2; a.g1 = g1; a.cslabs = cslabs; a.hslabs = hslabs;
        a.rows = std::min(p.C, M - m0); a.GC = p.GC; a.first = m0 == 0; a.key = train_key(nz, (uint32_t)m0);
        return a;
    }
    void fwd(int m0) { launch_enc_train_fwd(args(m0), st); }
    void bwd(int m0) { launch_enc_train_bwd(args(m0), st); }
    void close() {
        if (p.GC > 1) launch_slab_sum(cslabs, p.GC, ENC_CONV_P, grad, st);
        if (p.GH > 1) launch_slab_sum(hslabs, p.GH, ENC_HEAD_P, grad + ENC_CONV_P, st);
        ctx->last_macs += (int64_t)M * 3 * 3868960;     // forward, data gradient, weight gradient: 276 768 + 2 073 600 + 903 168 + 331 776 conv, 283 648 dense
    }
};

// efe_down_grad inside its call scope, for efe_train_down too (`who` names the entry point in the messages; grad: the caller's array, or the
// training call's scratch).  Every refusal comes before the first launch.
int down_grad_run(efe_ctx* ctx, const char* who, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, hipStream_t st) {
    const std::string w(who);
    if (M <= 0) return ctx->fail(w + ": M must be >= 1");
    if (!o1 || !ps1_mean || !ps1_logvar || !nz || !out || !grad)
        return ctx->fail(w + ": o1, ps1_mean, ps1_logvar, params, nz, out and grad must be non-NULL");
    if (fe_params(ctx, params, false, who)) return 1;
    if (!out->F_down) return ctx->fail(w + ": out->F_down is required");
    EncGrad e;
    if (e.open(ctx, who, o1, M, nz, out->qs1_mean, out->qs1_logvar, grad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st)) return 1;
    float* qs1 = out->qs1 ? out->qs1 : ctx->allocT<float>((size_t)M * S_DIM);
    float* d_s = ctx->allocT<float>((size_t)M * S_DIM);
    float* nl = out->nlogpo1 ? out->nlogpo1 : ctx->allocT<float>((size_t)M);
    float* gm = g_mean ? g_mean : ctx->allocT<float>((size_t)M * S_DIM);
    float* gv = g_logvar ? g_logvar : ctx->allocT<float>((size_t)M * S_DIM);
    if (!qs1 || !d_s || !nl || !gm || !gv) return 1;
    e.g_mean = gm; e.g_logvar = gv;
    const DecHeadIO hd{qs1, nz, d_s, nullptr, nullptr, nullptr, nullptr};
    DecGrad d;
    if (d.open(ctx, who, &hd, nullptr, nullptr, o1, M, -1.0f, params->beta_o, nl, out->po1, grad + ENC_P, nullptr, nullptr, nullptr, st)) return 1;
    const float* omega = params->omega_mode == EFE_OMEGA_ARRAY ? params->omega : nullptr;
    // F_down and its terms: k_fe_down's expressions on the training forward's po1, mean and logvar (nlogpo1 is the decoder group's own)
    efe_fe_out fo{};
    fo.F_down = out->F_down; fo.kl_s = out->kl_s; fo.kl_naive = out->kl_naive;
    FeArgs fa = fe_down_args(ctx, M, o1, e.mean, ps1_mean, ps1_logvar, S_DIM, params, omega, &fo);
    fa.q1_mean = e.mean; fa.q1_lv = e.logvar; fa.q1_ld = S_DIM;
    const uint32_t k0 = (uint32_t)nz->seed, k1 = (uint32_t)(nz->seed >> 32);
    for (int m0 = 0; m0 < M; m0 += e.p.C) {         // (both plans cut the rows at multiples of DEC_TAIL_ROWS)
        const int rows = d.rows(m0);
        const size_t r10 = (size_t)m0 * S_DIM;
        e.fwd(m0);
        launch_reparam(e.mean + r10, e.logvar + r10, eps ? eps + r10 : nullptr, qs1 + r10, rows, S_DIM, k0, k1, nz->pass, nz->sample, nz->stage,
                       nz->row_offset + (uint32_t)m0, st);
        d.group(m0);
        launch_fe_down(fa, d.po_of(m0), m0, rows, st);
        DownLatentArgs la{};
        la.d_s = d_s + r10; la.mean = e.mean + r10; la.logvar = e.logvar + r10; la.p1_mean = ps1_mean + r10; la.p1_lv = ps1_logvar + r10;
        la.eps_inj = eps ? eps + r10 : nullptr; la.omega_in = omega ? omega + m0 : nullptr; la.omega_scalar = params->omega_scalar;
        la.gamma = params->gamma; la.beta_s = params->beta_s; la.Mf = (float)M;
        la.g_mean = gm + r10; la.g_logvar = gv + r10; la.rows = rows; la.key = train_key(nz, (uint32_t)m0);
        launch_down_latent(la, st);
        e.bwd(m0);
    }
    d.close();
    e.close();
    return 0;
}

// ---- the same at every admitted geometry (train_enc_g.hip): EncGrad's shape with the sizes from the context ------------------------------
// Scratch of one row group from the arena: the activations the caller gives no output for, the four conv gradients, the S x rows x 256
// partials of W9 y4, g_0, and the two sets of slabs (none at G = 1: the gradient itself).  dW9 / db9 go into the gradient in place.
struct EncGradG {
    efe_ctx* ctx; const float* o; const float *g_mean, *g_logvar; int M; const efe_noise* nz;
    float *mean, *logvar, *grad, *y1, *y2, *y3, *y4, *h1, *h2, *h3;
    hipStream_t st;
    EncGeo geo;
    int C, GC, GH;
    float *s1, *s2, *s3, *s4, *a1, *a2, *a3, *g4, *g3, *g2, *g1, *part, *g0, *cslabs, *hslabs;
    // every refusal of the geometry-independent kind; M and the pointers are the caller's to check first
    int open(efe_ctx* ctx_, const char* who, const float* o_, int M_, const efe_noise* nz_, float* mean_, float* logvar_, float* grad_,
             float* y1_, float* y2_, float* y3_, float* y4_, float* h1_, float* h2_, float* h3_, hipStream_t st_) {
        ctx = ctx_; o = o_; M = M_; nz = nz_; mean = mean_; logvar = logvar_; grad = grad_;
        y1 = y1_; y2 = y2_; y3 = y3_; y4 = y4_; h1 = h1_; h2 = h2_; h3 = h3_; st = st_; g_mean = g_logvar = nullptr;
        const std::string w(who);
        if (!ctx->enc_raw_g) return ctx->fail(w + ": the weights are not committed");
        if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
        geo = EncGeo{ctx->chan, ctx->res};
        const DecTailGeo dg{ctx->base, ctx->chan, ctx->last_s1 ? 1 : 2};
        C = std::min(dg.rows_per_pass(), M); GC = enc_conv_slabs(M); GH = enc_head_slabs(M);
        const size_t n = (size_t)C;
        s1 = y1 ? nullptr : ctx->allocT<float>(n * geo.y1());
        s2 = y2 ? nullptr : ctx->allocT<float>(n * geo.y2());
        s3 = y3 ? nullptr : ctx->allocT<float>(n * geo.y3());
        s4 = y4 ? nullptr : ctx->allocT<float>(n * geo.y4());
        a1 = h1 ? nullptr : ctx->allocT<float>(n * 256);
        a2 = h2 ? nullptr : ctx->allocT<float>(n * 256);
        a3 = h3 ? nullptr : ctx->allocT<float>(n * 256);
        g4 = ctx->allocT<float>(n * geo.y4()); g3 = ctx->allocT<float>(n * geo.y3()); g2 = ctx->allocT<float>(n * geo.y2()); g1 = ctx->allocT<float>(n * geo.y1());
        part = ctx->allocT<float>((size_t)geo.segs() * n * 256);
        g0 = ctx->allocT<float>(n * 256);
        if (!mean) mean = ctx->allocT<float>((size_t)M * S_DIM);
        if (!logvar) logvar = ctx->allocT<float>((size_t)M * S_DIM);
        cslabs = GC > 1 ? ctx->allocT<float>((size_t)GC * geo.conv_P()) : grad;
        hslabs = GH > 1 ? ctx->allocT<float>((size_t)GH * ENC_SMALL_P) : grad + geo.small();
        if ((!y1 && !s1) || (!y2 && !s2) || (!y3 && !s3) || (!y4 && !s4) || (!h1 && !a1) || (!h2 && !a2) || (!h3 && !a3) || !g4 || !g3 || !g2 || !g1 ||
            !part || !g0 || !mean || !logvar || !cslabs || !hslabs)
            return 1;
        return 0;
    }
    EncTrainGArgs args(int m0) const {
        const size_t m = (size_t)m0;
        EncTrainGArgs a{};
        a.geo = geo; a.w = ctx->enc_raw_g; a.o = o + m * geo.img();
        a.y1 = y1 ? y1 + m * geo.y1() : s1; a.y2 = y2 ? y2 + m * geo.y2() : s2; a.y3 = y3 ? y3 + m * geo.y3() : s3; a.y4 = y4 ? y4 + m * geo.y4() : s4;
        a.h1 = h1 ? h1 + m * 256 : a1; a.h2 = h2 ? h2 + m * 256 : a2; a.h3 = h3 ? h3 + m * 256 : a3;
        a.mean = mean + m * S_DIM; a.logvar = logvar + m * S_DIM;
        a.g_mean = g_mean ? g_mean + m * S_DIM : nullptr; a.g_logvar = g_logvar ? g_logvar + m * S_DIM : nullptr;
        a.g4 = g4; a.g3 = g3; a.g2 = g2; a.g1 = g1; a.part = part; a.g0 = g0; a.grad = grad; a.cslabs = cslabs; a.hslabs = hslabs;
        a.rows = std::min(C, M - m0); a.GC = GC; a.first = m0 == 0; a.tile0 = m0 / 16; a.key = train_key(nz, (uint32_t)m0);
        return a;
    }
    void fwd(int m0) { launch_enc_train_g_fwd(args(m0), st); }
    void bwd(int m0) { launch_enc_train_g_bwd(args(m0), st); }
    void close() {
        if (GC > 1) launch_slab_sum(cslabs, GC, geo.conv_P(), grad, st);
        if (GH > 1) launch_slab_sum(hslabs, GH, ENC_SMALL_P, grad + geo.small(), st);
        // forward, data gradient, weight gradient: 288 C H1^2 + 9 216 H2^2 + 18 432 H3^2 + 36 864 H4^2 conv, 256 K + 2 x 65 536 + 5 120 dense
        const int64_t a1_ = geo.H1(), a2_ = geo.H2(), a3_ = geo.H3(), a4_ = geo.H4();
        ctx->last_macs += (int64_t)M * 3 * (288 * geo.C * a1_ * a1_ + 9216 * a2_ * a2_ + 18432 * a3_ * a3_ + 36864 * a4_ * a4_ + 256 * (int64_t)geo.K() + 136192);
    }
};

// efe_down_grad_g inside its call scope: down_grad_run's loop with the run-time-geometry encoder and decoder.  Every refusal comes before
// the first launch.
int down_grad_g_run(efe_ctx* ctx, const char* who, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                    const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, hipStream_t st) {
    const std::string w(who);
    if (M <= 0) return ctx->fail(w + ": M must be >= 1");
    if (!o1 || !ps1_mean || !ps1_logvar || !nz || !out || !grad)
        return ctx->fail(w + ": o1, ps1_mean, ps1_logvar, params, nz, out and grad must be non-NULL");
    if (fe_params(ctx, params, false, who)) return 1;
    if (!out->F_down) return ctx->fail(w + ": out->F_down is required");
    EncGradG e;
    if (e.open(ctx, who, o1, M, nz, out->qs1_mean, out->qs1_logvar, grad, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, st)) return 1;
    float* qs1 = out->qs1 ? out->qs1 : ctx->allocT<float>((size_t)M * S_DIM);
    float* d_s = ctx->allocT<float>((size_t)M * S_DIM);
    float* nl = out->nlogpo1 ? out->nlogpo1 : ctx->allocT<float>((size_t)M);
    float* gm = g_mean ? g_mean : ctx->allocT<float>((size_t)M * S_DIM);
    float* gv = g_logvar ? g_logvar : ctx->allocT<float>((size_t)M * S_DIM);
    if (!qs1 || !d_s || !nl || !gm || !gv) return 1;
    e.g_mean = gm; e.g_logvar = gv;
    const DecHeadIO hd{qs1, nz, d_s, nullptr, nullptr, nullptr, nullptr};
    DecGradG d;
    if (d.open(ctx, who, &hd, nullptr, o1, M, -1.0f, params->beta_o, nl, out->po1, nullptr, grad + e.geo.P(), nullptr, nullptr, nullptr, st)) return 1;
    const float* omega = params->omega_mode == EFE_OMEGA_ARRAY ? params->omega : nullptr;
    // F_down and its terms: k_fe_down's expressions on the training forward's po1 (NCHW here, whatever the context's forward store), mean and logvar
    efe_fe_out fo{};
    fo.F_down = out->F_down; fo.kl_s = out->kl_s; fo.kl_naive = out->kl_naive;
    FeArgs fa = fe_down_args(ctx, M, o1, e.mean, ps1_mean, ps1_logvar, S_DIM, params, omega, &fo);
    fa.q1_mean = e.mean; fa.q1_lv = e.logvar; fa.q1_ld = S_DIM; fa.nhwc4 = 0;
    const uint32_t k0 = (uint32_t)nz->seed, k1 = (uint32_t)(nz->seed >> 32);
    for (int m0 = 0; m0 < M; m0 += e.C) {           // (both cut the rows at multiples of rows_per_pass())
        const int rows = d.rows(m0);
        const size_t r10 = (size_t)m0 * S_DIM;
        e.fwd(m0);
        launch_reparam(e.mean + r10, e.logvar + r10, eps ? eps + r10 : nullptr, qs1 + r10, rows, S_DIM, k0, k1, nz->pass, nz->sample, nz->stage,
                       nz->row_offset + (uint32_t)m0, st);
        d.group(m0);
        launch_fe_down(fa, d.po_of(m0), m0, rows, st);
        DownLatentArgs la{};
        la.d_s = d_s + r10; la.mean = e.mean + r10; la.logvar = e.logvar + r10; la.p1_mean = ps1_mean + r10; la.p1_lv = ps1_logvar + r10;
        la.eps_inj = eps ? eps + r10 : nullptr; la.omega_in = omega ? omega + m0 : nullptr; la.omega_scalar = params->omega_scalar;
        la.gamma = params->gamma; la.beta_s = params->beta_s; la.Mf = (float)M;
        la.g_mean = gm + r10; la.g_logvar = gv + r10; la.rows = rows; la.key = train_key(nz, (uint32_t)m0);
        launch_down_latent(la, st);
        e.bwd(m0);
    }
    d.close();
    e.close();
    return 0;
}

// ModelDown's optimiser step (train_down.hip): the 1 x 64 x 64 geometry, exact fp32 planes only, sane hyper-parameters
int down_step_args(efe_ctx* ctx, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, DownAdamArgs& a, const char* who) {
    const std::string w(who);
    if (!exp_avg || !exp_avg_sq) return ctx->fail(w + ": exp_avg and exp_avg_sq must be non-NULL");
    if (ctx->chan != 1 || ctx->res != 64 || !ctx->down_master || !ctx->down_repack_n) return ctx->fail(w + ": built for the 1 x 64 x 64 geometry only");
    if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
    AdamArgs s{};
    if (adam_args(ctx, nullptr, hp, s, who)) return 1;
    a.m = exp_avg; a.v = exp_avg_sq; a.w = ctx->down_master; a.P = DOWN_P;
    a.omb1 = s.omb1; a.b2 = s.b2; a.omb2 = s.omb2; a.bc2_sqrt = s.bc2_sqrt; a.step_size = s.step_size; a.eps = s.eps;
    return 0;
}
// the update, then every packed forward form from the new raw copy; the host tensors and the host's copy of po_net.19.bias are stale from here,
// and so are split-operand planes left from a time the option was on (it is off now: down_step_args): marked unpacked, so that turning
// the option on again packs them from the trained weights (efe_set_option)
void down_step(efe_ctx* ctx, const DownAdamArgs& a, hipStream_t st) {
    ctx->down_dirty = true; ctx->dec_bf_stale = true; ctx->split_packed = 0;
    launch_adam_down(a, st);
    launch_repack_down(ctx->down_repack, ctx->down_repack_n, ctx->down_repack_blocks, ctx->down_master, st);
}

// efe_train_down inside its call scope, for efe_train_step too.  Every refusal comes before the first launch.
int train_down_run(efe_ctx* ctx, const char* who, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                   const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, hipStream_t st) {
    DownAdamArgs a{};
    if (down_step_args(ctx, exp_avg, exp_avg_sq, hp, a, who)) return 1;
    float* grad = ctx->allocT<float>((size_t)DOWN_P);
    if (!grad) return 1;
    if (down_grad_run(ctx, who, o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, nullptr, nullptr, grad, st)) return 1;
    a.g = grad;
    down_step(ctx, a, st);
    return 0;
}

// ---- ModelDown's optimiser step at every admitted geometry (train_down_g.hip behind k_adam_down) ------------------------------------------
// The step's arguments at the context's own geometry.  1 x 64 x 64: down_step_args (the one master copy and the one table of that geometry,
// shared with efe_train_down).  Else: the generic context's master copy, exact fp32 planes only, sane hyper-parameters.
int down_step_g_args(efe_ctx* ctx, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, DownAdamArgs& a, const char* who) {
    if (!ctx->generic) return down_step_args(ctx, exp_avg, exp_avg_sq, hp, a, who);
    const std::string w(who);
    if (!exp_avg || !exp_avg_sq) return ctx->fail(w + ": exp_avg and exp_avg_sq must be non-NULL");
    AdamArgs s{};
    if (adam_args(ctx, nullptr, hp, s, who)) return 1;
    if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
    if (!ctx->down_master_g || !ctx->down_repack_g_n) return ctx->fail(w + ": the weights are not committed");
    a.m = exp_avg; a.v = exp_avg_sq; a.w = ctx->down_master_g; a.P = (int)down_g_count(ctx);
    a.omb1 = s.omb1; a.b2 = s.b2; a.omb2 = s.omb2; a.bc2_sqrt = s.bc2_sqrt; a.step_size = s.step_size; a.eps = s.eps;
    return 0;
}
// the update, then every packed forward form of the context from the new master copy (down_step at 1 x 64 x 64); the host tensors and the
// host's copy of po_net.19.bias are stale from here
void down_step_g(efe_ctx* ctx, const DownAdamArgs& a, hipStream_t st) {
    if (!ctx->generic) { down_step(ctx, a, st); return; }
    ctx->down_dirty = true; ctx->g_bf_stale = true;
    launch_adam_down(a, st);
    launch_repack_down_g(ctx->down_repack_g, ctx->down_repack_g_n, ctx->down_repack_g_blocks, ctx->down_master_g, st);
}
// efe_train_down_g inside its call scope.  Every refusal comes before the first launch: M and the pointers first, then the step's own.
int train_down_g_run(efe_ctx* ctx, const char* who, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                     const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, hipStream_t st) {
    const std::string w(who);
    if (M <= 0) return ctx->fail(w + ": M must be >= 1");
    if (!o1 || !ps1_mean || !ps1_logvar || !params || !nz || !out || !exp_avg || !exp_avg_sq)
        return ctx->fail(w + ": o1, ps1_mean, ps1_logvar, params, nz, out, exp_avg and exp_avg_sq must be non-NULL");
    DownAdamArgs a{};
    if (down_step_g_args(ctx, exp_avg, exp_avg_sq, hp, a, who)) return 1;
    float* grad = ctx->allocT<float>((size_t)a.P);
    if (!grad) return 1;
    if (down_grad_g_run(ctx, who, o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, nullptr, nullptr, grad, st)) return 1;
    a.g = grad;
    down_step_g(ctx, a, st);
    return 0;
}
// the scope of a _g step's entry point did not open: an uncommitted context is refused under the entry point's name, like a stale handle
int step_g_refused(const Call& call, const char* who) {
    if (call.ctx && !call.ctx->committed) return call.ctx->fail(std::string(who) + ": weights not committed");
    return call.refused(who);
}

}  // namespace

extern "C" {

// ---- training of the habit net and the transition net (train.hip) -------------------------------------
int64_t efe_param_count(efe_ctx* ctx, const char* part) {
    Call call(ctx, Mode::host); if (!call) return 0;
    // the decoder's ConvTranspose2d tail po_net.13 / .15 / .17 / .19: a gradient exists (efe_dec_tail_grad), no optimiser step yet, so it is
    // no part of train_part()
    if (part && !strcmp(part, "po_net_convt")) return DT_B3 + 32 + 32 * ctx->chan * 9 + ctx->chan;
    // the whole decoder (efe_dec_grad), likewise without an optimiser step
    if (part && !strcmp(part, "po_net")) return DH_W3 + (int64_t)64 * ctx->base * ctx->base * 257 + DT_B3 + 32 + 32 * ctx->chan * 9 + ctx->chan;
    // the encoder (efe_enc_grad) and all of ModelDown, qs_net then po_net (efe_down_grad), at the one geometry those calls are built for
    if (part && (!strcmp(part, "qs_net") || !strcmp(part, "down"))) {
        if (ctx->chan != 1 || ctx->res != 64) { ctx->fail("efe_param_count: \"qs_net\" and \"down\" are counted for the 1 x 64 x 64 geometry only"); return 0; }
        return !strcmp(part, "qs_net") ? ENC_P : DOWN_P;
    }
    // the same two at the context's own geometry (efe_enc_grad_g, efe_down_grad_g).  "down_g" is also the length of the master copy and of the
    // optimiser state of efe_train_down_g / efe_down_adam_step_g / efe_down_get_weights_g
    if (part && (!strcmp(part, "qs_net_g") || !strcmp(part, "down_g")))
        return !strcmp(part, "qs_net_g") ? (int64_t)EncGeo{ctx->chan, ctx->res}.P() : down_g_count(ctx);
    if (!train_part(ctx, part, "efe_param_count")) return 0;
    return !strcmp(part, "top") ? part_param_count(TOP_NL, top_layer, ctx->pi_dim) : part_param_count(MID_NL, mid_layer, ctx->pi_dim);
}

int efe_get_weights(efe_ctx* ctx, const char* part, float* dst, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    const TrainPart* tp = train_part(ctx, part, "efe_get_weights"); if (!tp) return 1;
    if (!dst || n != tp->net.P) return ctx->fail("efe_get_weights: dst must hold efe_param_count(part) floats");
    HIPCHK(hipMemcpyAsync(dst, tp->master, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return call.finish();
}

int efe_top_grad(efe_ctx* ctx, const float* s, const float* log_Ppi, int M, float* kl_pi, float* grad, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!s || !log_Ppi || !grad || M < 1) return ctx->fail("efe_top_grad: bad arguments (s, log_Ppi and grad must be non-NULL, M >= 1)");
    TrainPart& tp = ctx->top_train;
    if (grad_or_step(ctx, tp, train_slabs(M), grad, nullptr, st, [&](float* slabs) {
            launch_top_grad(TopGradArgs{tp.net_dev, s, log_Ppi, kl_pi, slabs, M, ctx->pi_dim, 1.0f / (float)M}, st); })) return 1;
    return call.finish();
}

int efe_adam_step(efe_ctx* ctx, const char* part, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (!grad || !exp_avg || !exp_avg_sq) return ctx->fail("efe_adam_step: grad, exp_avg and exp_avg_sq must be non-NULL");
    TrainPart* tp = train_part(ctx, part, "efe_adam_step"); if (!tp) return 1;
    AdamArgs a{};
    if (adam_args(ctx, tp, hp, a, "efe_adam_step")) return 1;
    a.g = grad; a.nslab = 1; a.m = exp_avg; a.v = exp_avg_sq;
    tp->dirty = true;
    launch_adam(a, tp->net.P, st);
    return call.finish();
}

int efe_train_top(efe_ctx* ctx, const float* s, const float* log_Ppi, int M, float* kl_pi, float* exp_avg, float* exp_avg_sq,
                  const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (train_top_run(ctx, "efe_train_top", s, log_Ppi, M, kl_pi, exp_avg, exp_avg_sq, hp, st)) return 1;
    return call.finish();
}

int efe_mid_grad(efe_ctx* ctx, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                 const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* grad, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    MidGradArgs g{};
    if (mid_grad_args(ctx, s0, pi0, qs1_mean, qs1_logvar, M, params, nz, ps1_mean, ps1_logvar, F_mid, grad != nullptr, g, "efe_mid_grad")) return 1;
    if (grad_or_step(ctx, ctx->mid_train, train_mid_slabs(M), grad, nullptr, st, [&](float* slabs) { g.slabs = slabs; launch_mid_grad(g, st); })) return 1;
    return call.finish();
}

int efe_train_mid(efe_ctx* ctx, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp,
                  void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (train_mid_run(ctx, "efe_train_mid", s0, pi0, qs1_mean, qs1_logvar, M, params, nz, ps1_mean, ps1_logvar, F_mid, exp_avg, exp_avg_sq, hp, st)) return 1;
    return call.finish();
}

// ---- backward of the reconstruction loss through the decoder: ConvT tail (train_dec.hip), optionally behind the dense head (train_dec_head.hip) ----
int efe_dec_tail_grad(efe_ctx* ctx, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1, float* po1, float* d_h4,
                      float* grad, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (dec_grad(ctx, "efe_dec_tail_grad", nullptr, h4, d_h4, o1, M, scale, beta_o, nlogpo1, po1, grad, y1, y2, y3, st)) return 1;
    return call.finish();
}

int efe_dec_tail_grad_g(efe_ctx* ctx, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1, float* po1, float* d_h4,
                        float* grad, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_dec_tail_grad_g");
    if (dec_grad_g_run(ctx, "efe_dec_tail_grad_g", nullptr, h4, o1, M, scale, beta_o, nlogpo1, po1, d_h4, grad, y1, y2, y3, st)) return 1;
    return call.finish();
}

int efe_dec_grad(efe_ctx* ctx, const float* s, const float* o1, int M, float scale, float beta_o, const efe_noise* nz, float* nlogpo1, float* po1,
                 float* d_s, float* grad, float* h1, float* h2, float* h3, float* h4, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    const DecHeadIO hd{s, nz, d_s, h1, h2, h3, h4};
    if (dec_grad(ctx, "efe_dec_grad", &hd, nullptr, nullptr, o1, M, scale, beta_o, nlogpo1, po1, grad, y1, y2, y3, st)) return 1;
    return call.finish();
}

int efe_dec_grad_g(efe_ctx* ctx, const float* s, const float* o1, int M, float scale, float beta_o, const efe_noise* nz, float* nlogpo1, float* po1,
                   float* d_s, float* grad, float* h1, float* h2, float* h3, float* h4, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_dec_grad_g");
    const DecHeadIO hd{s, nz, d_s, h1, h2, h3, h4};
    if (dec_grad_g_run(ctx, "efe_dec_grad_g", &hd, nullptr, o1, M, scale, beta_o, nlogpo1, po1, nullptr, grad, y1, y2, y3, st)) return 1;
    return call.finish();
}

int efe_enc_grad(efe_ctx* ctx, const float* o, const float* g_mean, const float* g_logvar, int M, const efe_noise* nz, float* mean, float* logvar,
                 float* grad, float* y1, float* y2, float* y3, float* y4, float* h1, float* h2, float* h3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (M <= 0) return ctx->fail("efe_enc_grad: M must be >= 1");
    if (!o || !g_mean || !g_logvar || !nz || !grad) return ctx->fail("efe_enc_grad: o, g_mean, g_logvar, nz and grad must be non-NULL");
    EncGrad e;
    if (e.open(ctx, "efe_enc_grad", o, M, nz, mean, logvar, grad, y1, y2, y3, y4, h1, h2, h3, st)) return 1;
    e.g_mean = g_mean; e.g_logvar = g_logvar;
    for (int m0 = 0; m0 < M; m0 += e.p.C) { e.fwd(m0); e.bwd(m0); }
    e.close();
    return call.finish();
}

int efe_down_grad(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (down_grad_run(ctx, "efe_down_grad", o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, g_mean, g_logvar, grad, st)) return 1;
    return call.finish();
}

int efe_enc_grad_g(efe_ctx* ctx, const float* o, const float* g_mean, const float* g_logvar, int M, const efe_noise* nz, float* mean, float* logvar,
                   float* grad, float* y1, float* y2, float* y3, float* y4, float* h1, float* h2, float* h3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_enc_grad_g");
    if (M <= 0) return ctx->fail("efe_enc_grad_g: M must be >= 1");
    if (!o || !g_mean || !g_logvar || !nz || !grad) return ctx->fail("efe_enc_grad_g: o, g_mean, g_logvar, nz and grad must be non-NULL");
    EncGradG e;
    if (e.open(ctx, "efe_enc_grad_g", o, M, nz, mean, logvar, grad, y1, y2, y3, y4, h1, h2, h3, st)) return 1;
    e.g_mean = g_mean; e.g_logvar = g_logvar;
    for (int m0 = 0; m0 < M; m0 += e.C) { e.fwd(m0); e.bwd(m0); }
    e.close();
    return call.finish();
}

int efe_down_grad_g(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                    const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_down_grad_g");
    if (down_grad_g_run(ctx, "efe_down_grad_g", o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, g_mean, g_logvar, grad, st)) return 1;
    return call.finish();
}

int efe_train_down(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                   const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_train_down");
    if (train_down_run(ctx, "efe_train_down", o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, exp_avg, exp_avg_sq, hp, st)) return 1;
    return call.finish();
}

// ---- one whole training step (train.py:111-126): the three run functions behind the two encoder passes, omega formed on the device ---------
int efe_train_step(efe_ctx* ctx, const efe_step_in* in, int M, const efe_fe_params* params, const efe_noise* nz, const efe_step_adam* top,
                   const efe_step_adam* mid, const efe_step_adam* down, const efe_step_out* out, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_train_step");
    const char* who = "efe_train_step";
    // every refusal before the first launch: what the run functions below would refuse, checked for all three parts up front
    if (M < 1) return ctx->fail("efe_train_step: M must be >= 1");
    if (!in || !in->o0 || !in->o1 || !in->pi0 || !in->log_Ppi || !nz || !out || !out->kl_pi || !out->F_down)
        return ctx->fail("efe_train_step: in (o0, o1, pi0, log_Ppi), params, nz and out (kl_pi, F_down) must be non-NULL");
    if (!top || !mid || !down || !top->exp_avg || !top->exp_avg_sq || !mid->exp_avg || !mid->exp_avg_sq || !down->exp_avg || !down->exp_avg_sq)
        return ctx->fail("efe_train_step: top, mid and down with their exp_avg and exp_avg_sq must be non-NULL");
    if (fe_params(ctx, params, true, who)) return 1;
    {
        AdamArgs a{}; DownAdamArgs d{};
        if (adam_args(ctx, &ctx->top_train, &top->hp, a, "efe_train_step (top)") || adam_args(ctx, &ctx->mid_train, &mid->hp, a, "efe_train_step (mid)")) return 1;
        if (down_step_args(ctx, down->exp_avg, down->exp_avg_sq, &down->hp, d, "efe_train_step (down)")) return 1;      // (geometry, split-operand options)
        if (!ctx->enc_raw || !ctx->dec_raw) return ctx->fail("efe_train_step (down): built for the 1 x 64 x 64 geometry only");
    }
    const uint32_t k0 = (uint32_t)nz->seed, k1 = (uint32_t)(nz->seed >> 32);
    const float* eps_q0 = in->eps;
    const float* eps_d = in->eps ? in->eps + (size_t)2 * M * S_DIM : nullptr;
    // what outlives a part: the arrays the caller does not want stand in scratch; each part's own scratch is handed back behind it (the
    // stream orders the parts, as it orders fe_down's chunks)
    auto own = [&](float* p, size_t n) { return p ? p : ctx->allocT<float>(n); };
    float* qs0 = own(out->qs0, (size_t)M * S_DIM);
    float* omega = own(out->omega, (size_t)M);
    float* qm = ctx->allocT<float>((size_t)M * S_DIM);
    float* qv = ctx->allocT<float>((size_t)M * S_DIM);
    float* pm = own(out->ps1_mean, (size_t)M * S_DIM);
    float* pv = own(out->ps1_logvar, (size_t)M * S_DIM);
    float* F_mid = own(out->F_mid, (size_t)M);
    float* nl = out->means ? own(out->nlogpo1, (size_t)M) : out->nlogpo1;
    float* kls = out->means ? own(out->kl_s, (size_t)M) : out->kl_s;
    float* kln = out->means ? own(out->kl_naive, (size_t)M) : out->kl_naive;
    if (!qs0 || !omega || !qm || !qv || !pm || !pv || !F_mid || (out->means && (!nl || !kls || !kln))) return 1;
    const Arena::Mark mark = ctx->arena.mark();
    efe_noise pz = *nz; pz.sample = 0;
    // 1. qs0 = encoder_with_sample(o0): efe_encoder under PASS_FE_Q0
    {
        float* enc = ctx->allocT<float>((size_t)M * 32);
        if (!enc) return 1;
        if (run_encoder(ctx, in->o0, M, pass_noise(nz, PASS_FE_Q0, 0, M), enc, st)) return 1;
        launch_root_post(enc, nullptr, eps_q0, nullptr, qs0, M, 0, k0, k1, PASS_FE_Q0, 0, nz->stage, nz->row_offset, ctx->pi_dim, st);
    }
    // 2. the habit net's step
    if (train_top_run(ctx, "efe_train_step (top)", qs0, in->log_Ppi, M, out->kl_pi, top->exp_avg, top->exp_avg_sq, &top->hp, st)) return 1;
    ctx->arena.rewind(mark);
    // 3. omega: compute_omega(kl_pi) of this call, or the caller's
    {
        FeArgs a{};
        a.M = M; a.kl_pi = out->kl_pi;
        fe_omega(a, params); a.omega_out = omega;
        launch_step_omega(a, st);
    }
    efe_fe_params pw = *params;
    pw.omega_mode = EFE_OMEGA_ARRAY; pw.omega = omega;
    // 4. qs1_mean, qs1_logvar = encoder(o1): efe_encoder under PASS_FE_Q1
    {
        float* enc = ctx->allocT<float>((size_t)M * 32);
        if (!enc) return 1;
        if (run_encoder(ctx, in->o1, M, pass_noise(nz, PASS_FE_Q1, 0, M), enc, st)) return 1;
        launch_split_enc(enc, qm, qv, M, st);
    }
    // 5. the transition net's step
    pz.pass = PASS_FE_T;
    if (train_mid_run(ctx, "efe_train_step (mid)", qs0, in->pi0, qm, qv, M, &pw, &pz, pm, pv, F_mid, mid->exp_avg, mid->exp_avg_sq, &mid->hp, st)) return 1;
    ctx->arena.rewind(mark);
    // 6. ModelDown's step
    pz.pass = PASS_FE_DOWN;
    efe_fe_out fo{};
    fo.F_down = out->F_down; fo.nlogpo1 = nl; fo.kl_s = kls; fo.kl_naive = kln;
    if (train_down_run(ctx, "efe_train_step (down)", in->o1, pm, pv, M, &pw, &pz, eps_d, &fo, down->exp_avg, down->exp_avg_sq, &down->hp, st)) return 1;
    if (out->means) launch_step_means(StepMeansArgs{{out->kl_pi, omega, F_mid, out->F_down, nl, kls, kln}, out->means, M}, st);
    return call.finish();
}

int efe_down_adam_step(efe_ctx* ctx, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_down_adam_step");
    if (!grad) return ctx->fail("efe_down_adam_step: grad must be non-NULL");
    DownAdamArgs a{};
    if (down_step_args(ctx, exp_avg, exp_avg_sq, hp, a, "efe_down_adam_step")) return 1;
    a.g = grad;
    down_step(ctx, a, st);
    return call.finish();
}

int efe_train_down_g(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                     const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return step_g_refused(call, "efe_train_down_g");
    if (train_down_g_run(ctx, "efe_train_down_g", o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, exp_avg, exp_avg_sq, hp, st)) return 1;
    return call.finish();
}

int efe_down_adam_step_g(efe_ctx* ctx, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return step_g_refused(call, "efe_down_adam_step_g");
    if (!grad) return ctx->fail("efe_down_adam_step_g: grad must be non-NULL");
    DownAdamArgs a{};
    if (down_step_g_args(ctx, exp_avg, exp_avg_sq, hp, a, "efe_down_adam_step_g")) return 1;
    a.g = grad;
    down_step_g(ctx, a, st);
    return call.finish();
}

int efe_down_get_weights_g(efe_ctx* ctx, float* dst, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return step_g_refused(call, "efe_down_get_weights_g");
    const float* master = ctx->generic ? ctx->down_master_g : ctx->down_master;
    if (!master) return ctx->fail("efe_down_get_weights_g: the weights are not committed");
    if (!dst || n != down_g_count(ctx)) return ctx->fail("efe_down_get_weights_g: dst must hold efe_param_count(\"down_g\") floats");
    HIPCHK(hipMemcpyAsync(dst, master, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return call.finish();
}

int efe_down_get_weights(efe_ctx* ctx, float* dst, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_down_get_weights");
    if (ctx->chan != 1 || ctx->res != 64 || !ctx->down_master) return ctx->fail("efe_down_get_weights: built for the 1 x 64 x 64 geometry only");
    if (!dst || n != DOWN_P) return ctx->fail("efe_down_get_weights: dst must hold efe_param_count(\"down\") floats");
    HIPCHK(hipMemcpyAsync(dst, ctx->down_master, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return call.finish();
}

}  // extern "C"
