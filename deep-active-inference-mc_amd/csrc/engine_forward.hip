// Host side of the engine, the forward passes: the launch helpers, the scratch plans, and the runners of the four networks and of
// calculate_G (run_core), which the entry points of engine_efe.hip, engine_loss.hip and engine_train.hip call.  No entry point of its own.
#include "engine.h"

namespace efe {
namespace host {
namespace {

// ---- launch helpers ----------------------------------------------------------------------------------
inline RowMask live_of(const NoiseCfg& nc, int m0) { return RowMask{nc.mask, nc.mask_div, m0, nc.rows_per_group, nc.mask ? nc.gm.ids : nullptr}; }
// the six noise-addressing fields that GemmArgs, HeadArgs and TransFusedArgs share by name
template <class Args>
void set_keys(Args& a, const NoiseCfg& nc, int m0) {
    a.k0 = nc.k0; a.k1 = nc.k1; a.gm = nc.gm; a.rows_per_group = nc.rows_per_group; a.row_offset = nc.row_offset; a.m0 = m0;
}

// split16 = false: the decoder's Linear(256, 16384) stays on the exact fp32 k_fc4 even under a split-operand option (its consumer is fp32)
void fc(efe_ctx* ctx, int cls, const Layer& L, const float* X, int ldx, int x_mod, float* Y, int ldy, int M, bool relu, bool drop,
        uint32_t tag, const NoiseCfg& nc, int m0, hipStream_t st, bool split16 = true) {
    GemmArgs a{};
    a.Wp = L.Wp; a.bias = L.bias; a.X = X; a.Y = Y; a.zeros = ctx->zeros;
    a.n_pix = M; a.cin = L.cin; a.cout = L.cout; a.mtiles = L.mtiles; a.ldx = ldx; a.ldy = ldy; a.x_mod = x_mod;
    a.relu = relu; a.dropout = drop; a.tag = tag;
    set_keys(a, nc, m0);
    ProfSpan span(ctx, cls, st);
    if (L.mtiles >= 64 && !(L.mtiles & 1) && L.cin == 256 && ldx == 256 && x_mod == 0 && relu && drop) {
        if (split16 && ctx->mfma_bf16x3 && ctx->fc4_b3 && &L == &ctx->dec_fc[3]) {      // opt-in experiment
            a.Wb3 = ctx->fc4_b3; a.split = (int)ctx->mfma_bf16x3; a.wb3_scale_inv = 1.0f / ctx->s_fc4;
            launch_fc4_b3(a, st);
        }
        else launch_fc4(a, st);     // Linear(256, 64 * base^2): batch tile staged in LDS
    } else {
        // tile shape by problem size: small launches (transition / habit / heads) use 32x32 wave tiles so that the
        // grid still covers the 256 CUs
        int MT = L.mtiles == 1 ? 1 : 2, NT = 2;
        const long tiles22 = (long)((L.mtiles + MT - 1) / MT) * ((M + 63) / 64);
        if (tiles22 < 2048) { NT = 1; if (tiles22 * 2 < 2048) MT = 1; }
        if (launch_dense(MT, NT, a, st)) ctx->pending = "launch_dense: unsupported tile shape";
    }
}

// The dense head of the decoder (enc = false: X [M][16] -> out [M][256], three layers) or of the encoder (X [M][ldx] -> out [M][32], four
// layers): one launch (fused.hip k_head), or layer by layer through hA / hB ([M][256] each) under the option head_unfused
void dense_head(efe_ctx* ctx, bool enc, const float* X, int ldx, float* out, int ldy, float* hA, float* hB, int M, const NoiseCfg& nc, int m0,
                hipStream_t st) {
    const int cls = enc ? PROF_ENC : PROF_DEC_FC;
    const uint32_t tag = enc ? TAG_ENC : TAG_DEC;
    if (!ctx->head_unfused) {
        HeadArgs a{};
        a.W = enc ? ctx->enc16 : ctx->dec16; a.kc0 = enc ? ctx->enc16_kc0 : 1; a.nl = enc ? 4 : 3; a.out_tiles = 2;
        a.tag0 = tag; a.X = X; a.Y = out; a.M = M;
        set_keys(a, nc, m0);
        ProfSpan span(ctx, cls, st);
        launch_head(a, st);
        return;
    }
    const Layer* L = enc ? ctx->enc_fc : ctx->dec_fc;
    fc(ctx, cls, L[0], X, ldx, 0, hA, 256, M, true, true, tag + 0, nc, m0, st);
    fc(ctx, cls, L[1], hA, 256, 0, hB, 256, M, true, true, tag + 1, nc, m0, st);
    if (!enc) { fc(ctx, cls, L[2], hB, 256, 0, out, ldy, M, true, true, tag + 2, nc, m0, st); return; }
    fc(ctx, cls, L[2], hB, 256, 0, hA, 256, M, true, true, tag + 2, nc, m0, st);
    fc(ctx, cls, L[3], hA, 256, 0, out, ldy, M, false, false, 0, nc, m0, st);
}

// one layer of the generic geometry on k_conv_g: mode 0 = Conv2d(k3, s2, p0), 1 / 2 = ConvTranspose2d of stride 1 / 2; square images, + ReLU
void conv_g(efe_ctx* ctx, int cls, const Layer& L, const float* in, float* out, int n, int hin, int cin, int hout, int cout, int mode,
            const RowMask& live, hipStream_t st) {
    ConvGArgs a{};
    a.in = in; a.out = out; a.Wp = L.Wp; a.bias = L.bias; a.zeros = ctx->zeros; a.n_img = n; a.Hin = hin; a.Win = hin; a.Cin = cin;
    a.Hout = hout; a.Wout = hout; a.Cout = cout; a.mtiles = L.mtiles; a.mode = mode; a.relu = 1; a.ldo = cout;
    a.live = live;
    ProfSpan span(ctx, cls, st);
    launch_conv_g(a, st);
}

// ---- scratch plans -----------------------------------------------------------------------------------
// Every path that takes scratch describes its buffers ONCE, as a plan: a pure function of the context's options and the call's sizes that
// returns the element count of each buffer (all are 4-byte elements; 0 = the buffer does not exist) and whatever decides a count (chunk
// sizes, which kernels run).  run_X allocates from its plan, in the order of the plan's fields; efe_rollout_scratch_bytes sums the same
// plans (plan_bytes: what the arena charges for them).
size_t arena_bytes(const efe_ctx* ctx, std::initializer_list<size_t> counts) {
    size_t t = 0;
    for (size_t n : counts) t += ctx->al(n * 4);
    return t;
}

struct MidPlan { size_t h1, h2; };      // layer-by-layer transition only (option mid_unfused)
MidPlan mid_plan(const efe_ctx* ctx, int64_t M) { const size_t h = ctx->mid_unfused ? (size_t)M * 512 : 0; return {h, h}; }
size_t plan_bytes(const efe_ctx* c, const MidPlan& p) { return arena_bytes(c, {p.h1, p.h2}); }

// does the generic decoder run its last two layers as k_dec_bg?  Decided from the geometry (y3 exists only when the final layer is its own launch)
bool generic_dec_fused(const efe_ctx* ctx) { return ctx->fuse_final_g && !ctx->last_s1 && dec_bg_ok(2 * ctx->base, 2 * ctx->base, ctx->chan); }
struct DecGPlan { int C; bool fused; size_t hA, hB, x4, y1, y2, y3; };      // C: images per launch group; fused: last two layers in one kernel
DecGPlan dec_g_plan(const efe_ctx* ctx, int64_t N) {
    const int64_t B = ctx->base, H2 = 2 * B, H3 = ctx->last_s1 ? 2 * B : 4 * B;
    DecGPlan p{};
    p.fused = generic_dec_fused(ctx);
    // images per launch group: bounded by the chunk options and by a byte budget for the group's layer activations
    const int64_t per_image = (2 * B * B * 64 + H2 * H2 * 64 + (p.fused ? 0 : H3 * H3 * 32)) * (int64_t)sizeof(float);
    const int64_t by_bytes = std::max<int64_t>(256, ctx->dec_budget_g / per_image);
    const int64_t C = std::min<int64_t>(std::min<int64_t>(std::min<int64_t>(ctx->dec_chunk, ctx->dec_chunk_g), by_bytes), N);
    p.C = (int)C;
    p.hA = p.hB = (size_t)N * 256;
    p.x4 = p.y1 = (size_t)(C * B * B * 64);
    p.y2 = (size_t)(C * H2 * H2 * 64);
    p.y3 = p.fused ? 0 : (size_t)(C * H3 * H3 * 32);
    return p;
}
size_t plan_bytes(const efe_ctx* c, const DecGPlan& p) { return arena_bytes(c, {p.hA, p.hB, p.x4, p.y1, p.y2, p.y3}); }

// dSprites decoder: launches of at most this many images split every image over four workgroups in k_dec_b4 (per-image sums as quarters, valq)
constexpr int DEC_SPLIT_MAX = 128;
inline bool dec_split(const efe_ctx* ctx, int64_t N) { return !ctx->generic && ctx->dec_split && N <= DEC_SPLIT_MAX; }
// Option dec_fuse_ab: the large-launch fp32 kernels k_dec_a and k_dec_b4<1> as one persistent launch, k_dec_ab, whose workgroups keep y2 in
// a slot of their own (DecPlan::grid slots of 256 KiB instead of one per image of a launch group).  A fused launch has no boundary between
// the profiling classes dec_a_convT1_convT2 and dec_b_convT3_final_reduce: while either is being timed, the call runs the two launches.
inline bool dec_fused(const efe_ctx* ctx, int64_t N) {
    return !ctx->generic && ctx->dec_fuse_ab && !dec_split(ctx, N) && !ctx->mfma_bf16x3 && !(ctx->prof & ((1u << PROF_CT2) | (1u << PROF_CT3)));
}
struct DecPlan { int C; bool split, fused; int grid; size_t hA, hB, x4, y2, queues; };       // queues: one image-ticket counter (int) per k_dec_a / k_dec_ab launch
DecPlan dec_plan(const efe_ctx* ctx, int64_t N) {
    const int64_t C = std::min<int64_t>(ctx->dec_chunk, N);
    const bool fused = dec_fused(ctx, N);
    const int grid = fused ? dec_ab_grid((int)C, (int)ctx->dec_ab_grid) : 0;
    return {(int)C, dec_split(ctx, N), fused, grid, (size_t)N * 256, (size_t)N * 256, (size_t)C * 16384, (size_t)(fused ? grid : C) * 65536,
            (size_t)((N + C - 1) / C)};
}
size_t plan_bytes(const efe_ctx* c, const DecPlan& p) { return arena_bytes(c, {p.hA, p.hB, p.x4, p.y2, p.queues}); }

// widen: layer 1 runs on k_conv_g, which reads 8-channel pixels from o8w.  The buffer is taken on first use and the plan foresees the option
// enc_tiled = 0 only: kernels.h has no predicate that tells beforehand whether k_conv_e declines a geometry (none that efe_create_cfg admits is)
struct EncGPlan { int C; bool widen; size_t c1, c2, c3, c4, hA, hB, o8w; };
EncGPlan enc_g_plan(const efe_ctx* ctx, int64_t N) {
    const int* hw = ctx->enc_hw;
    const size_t C = (size_t)std::min<int64_t>(std::min<int64_t>(ctx->enc_chunk, 8192), N);
    return {(int)C, ctx->enc_tiled == 0, C * hw[1] * hw[1] * 32, C * hw[2] * hw[2] * 32, C * hw[3] * hw[3] * 64, C * hw[4] * hw[4] * 64,
            C * 256, C * 256, C * hw[0] * hw[0] * 8};
}
size_t plan_bytes(const efe_ctx* c, const EncGPlan& p) { return arena_bytes(c, {p.c1, p.c2, p.c3, p.c4, p.hA, p.hB, p.widen ? p.o8w : 0}); }

struct EncPlan { int C; size_t c4, hA, hB; };
EncPlan enc_plan(const efe_ctx* ctx, int64_t N) { const size_t C = (size_t)std::min<int64_t>(ctx->enc_chunk, N); return {(int)C, C * 9 * 64, C * 256, C * 256}; }
size_t plan_bytes(const efe_ctx* c, const EncPlan& p) { return arena_bytes(c, {p.c4, p.hA, p.hB}); }

// run_core over R rows, D stages, S samples: own_tr = the transition rows are not the caller's (k_sim_chain's), own_terms = no `terms` output given;
// vsplit: a small decoder launch, whose per-image sums arrive as four quarter sums
struct CorePlan { bool vsplit; size_t tr_all, dec_in, xbuf, val, po_store, enc, terms_tmp; };
CorePlan core_plan(const efe_ctx* ctx, int64_t R_, int64_t D_, int64_t S_, bool own_tr, bool own_terms) {
    const size_t R = (size_t)R_, D = (size_t)D_, S = (size_t)S_;
    const bool vsplit = dec_split(ctx, D_ * 3 * S_ * R_);
    return {vsplit, own_tr ? D * 2 * S * R * 32 : 0, D * 3 * S * R * 16, 2 * R * 16, D * 3 * S * R * (vsplit ? 4 : 1), D * S * R * ctx->img_store,
            D * S * R * 32, own_terms ? 3 * R : 0};
}
size_t plan_bytes(const efe_ctx* c, const CorePlan& p) { return arena_bytes(c, {p.tr_all, p.dec_in, p.xbuf, p.val, p.po_store, p.enc, p.terms_tmp}); }

size_t plan_bytes(const efe_ctx* c, const DecTailPlan& p) { return arena_bytes(c, {p.y1, p.y2, p.y3, p.po, p.g4, p.g3, p.g2, p.g1, p.slabs}); }

// the sums, nested as the calls are: run_decoder / run_encoder dispatch on the geometry, run_core runs D transitions and one pass of each
size_t decoder_bytes(const efe_ctx* ctx, int64_t N) { return ctx->generic ? plan_bytes(ctx, dec_g_plan(ctx, N)) : plan_bytes(ctx, dec_plan(ctx, N)); }

// generic geometry (generic.hip): dense head -> Linear(256, 64*B*B) -> ConvT(64,64,s1) -> ConvT(64,64,s2) -> ConvT(64,32,s2) -> final conv
int run_decoder_g(efe_ctx* ctx, const float* dec_in, int N, const NoiseCfg& nc, int reward0, int store0, float* val, float* po_store,
                  hipStream_t st) {
    const int B = ctx->base, H2 = 2 * B, H3 = ctx->last_s1 ? 2 * B : 4 * B;
    // po_net.19.bias goes to k_dec_bg / k_final_g by value: after a device-side optimiser step (efe_train_down_g / efe_down_adam_step_g) the
    // host floats are stale, and the first decoder pass behind the step fetches them from the master copy's tail on its own stream, once
    // (run_decoder's rule for dec_bf)
    if (ctx->g_bf_stale) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return ctx->fail("decoder: the first pass after an optimiser step of ModelDown synchronises its stream once and cannot be captured");
        const int64_t P = down_g_count(ctx);
        if (!ctx->down_master_g || hipMemcpyAsync(ctx->g_bf, ctx->down_master_g + P - ctx->chan, (size_t)ctx->chan * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return ctx->fail("decoder: fetching po_net.19.bias after an optimiser step failed");
        ctx->g_bf_stale = false;
    }
    const DecGPlan p = dec_g_plan(ctx, N);
    const int C = p.C;
    float* hA = ctx->allocT<float>(p.hA);
    float* hB = ctx->allocT<float>(p.hB);
    float* x4 = ctx->allocT<float>(p.x4);
    float* y1 = ctx->allocT<float>(p.y1);
    float* y2 = ctx->allocT<float>(p.y2);
    float* y3 = p.fused ? nullptr : ctx->allocT<float>(p.y3);
    if (!hA || !hB || !x4 || !y1 || !y2 || (!p.fused && !y3)) return 1;
    ctx->last_macs += (int64_t)N * ctx->mac_dec;
    dense_head(ctx, false, dec_in, 16, hA, 256, hA, hB, N, nc, 0, st);
    for (int m0 = 0; m0 < N; m0 += C) {
        const int c = std::min(C, N - m0);
        const RowMask live = live_of(nc, m0);
        fc(ctx, PROF_DEC_FC4, ctx->g_fc4, hA + (size_t)m0 * 256, 256, 0, x4, B * B * 64, c, true, true, TAG_DEC + 3, nc, m0, st);
        int sep12 = 1;                                    // the first two transposed layers as one launch each
        if (ctx->ct_fuse12) {                             // ... or as one kernel, layer 1's output kept in LDS (class PROF_CT2)
            ConvT12Args f{};
            f.in = x4; f.out = y2; f.W1p = ctx->g_ct[0].Wp; f.b1 = ctx->g_ct[0].bias; f.W2p = ctx->g_ct[1].Wp; f.b2 = ctx->g_ct[1].bias;
            f.n_img = c; f.Hin = B; f.Win = B; f.live = live;
            ProfSpan span(ctx, PROF_CT2, st);
            sep12 = launch_convt_12(f, st);
            if (sep12) span.cancel();
        }
        if (sep12) {
            conv_g(ctx, PROF_CT1, ctx->g_ct[0], x4, y1, c, B, 64, B, 64, 1, live, st);
            conv_g(ctx, PROF_CT2, ctx->g_ct[1], y1, y2, c, B, 64, H2, 64, 2, live, st);
        }
        if (p.fused) {      // ConvT(64,32,s2) + ReLU + ConvT(32,C,s1) + Sigmoid + per-image sums in one kernel: y3 never exists
            DecBGArgs f{};
            f.y2 = y2; f.w3 = ctx->g_ct[2].Wp; f.b3 = ctx->g_ct[2].bias; f.w4 = ctx->g_wf; for (int i = 0; i < 4; ++i) f.b4[i] = ctx->g_bf[i];
            f.rows = c; f.m0 = m0; f.rows_per_group = nc.rows_per_group; f.Hin = H2; f.Win = H2; f.C = ctx->chan; f.gm = nc.gm;
            f.reward0 = reward0; f.store0 = store0; f.reward_intent = (int)ctx->reward_intent; f.val = val; f.po = po_store; f.live = live;
            ProfSpan span(ctx, PROF_CT3, st);
            if (launch_dec_bg(f, st)) return ctx->fail("fused decoder tail: unsupported geometry");      // (dec_bg_ok said yes: not reachable)
            continue;
        }
        conv_g(ctx, PROF_CT3, ctx->g_ct[2], y2, y3, c, H2, 64, H3, 32, ctx->last_s1 ? 1 : 2, live, st);
        FinalGArgs f{};
        f.y3 = y3; f.w = ctx->g_wf; for (int i = 0; i < 4; ++i) f.b[i] = ctx->g_bf[i];
        f.rows = c; f.m0 = m0; f.rows_per_group = nc.rows_per_group; f.H = H3; f.W = H3; f.C = ctx->chan; f.gm = nc.gm;
        f.reward0 = reward0; f.store0 = store0; f.reward_intent = (int)ctx->reward_intent; f.val = val; f.po = po_store; f.live = live;
        ProfSpan span(ctx, PROF_FINAL, st);
        if (launch_final_g(f, st)) return ctx->fail("final decoder layer: unsupported geometry");
    }
    return 0;
}

// generic geometry: o is NHWC4 [N][res*res][4]; four Conv2d(k3,s2,p0)+ReLU, then the dense head
int run_encoder_g(efe_ctx* ctx, const float* o8, int N, const NoiseCfg& nc, float* enc, hipStream_t st) {
    const int* hw = ctx->enc_hw;
    const EncGPlan p = enc_g_plan(ctx, N);
    const int C = p.C;
    float* c1 = ctx->allocT<float>(p.c1);
    float* c2 = ctx->allocT<float>(p.c2);
    float* c3 = ctx->allocT<float>(p.c3);
    float* c4 = ctx->allocT<float>(p.c4);
    float* hA = ctx->allocT<float>(p.hA);
    float* hB = ctx->allocT<float>(p.hB);
    if (!c1 || !c2 || !c3 || !c4 || !hA || !hB) return 1;
    ctx->last_macs += (int64_t)N * ctx->mac_enc;
    const int flat = hw[4] * hw[4] * 64;
    float* o8w = nullptr;
    for (int m0 = 0; m0 < N; m0 += C) {
        const int c = std::min(C, N - m0);
        const RowMask live = live_of(nc, m0);
        // layers 1 and 2 LDS-tiled (generic_enc.hip); k_conv_g where a geometry is outside that kernel's limits
        auto conv_e = [&](int layer, const float* in, float* out, const float* Wp, const float* bias, int hin, int hout) -> int {
            ConvEArgs e{};
            e.in = in; e.out = out; e.Wp = Wp; e.bias = bias; e.n_img = c; e.Hin = hin; e.Win = hin; e.Hout = hout; e.Wout = hout;
            e.live = live;
            ProfSpan span(ctx, PROF_ENC, st);
            const int rc = ctx->enc_tiled ? launch_conv_e(e, layer, st) : 1;
            if (rc) span.cancel();
            return rc;
        };
        const float* o4c = o8 + (size_t)m0 * hw[0] * hw[0] * GEN_IMG_LD;
        int sep12 = 1;                                    // layers 1 and 2 as one launch each
        if (ctx->enc_tiled >= 2) {                        // ... or as one kernel, conv1's output kept in LDS
            ConvE12Args e{};
            e.in = o4c; e.out = c2; e.W1p = ctx->g_enc1p; e.b1 = ctx->g_enc[0].bias; e.W2p = ctx->g_enc[1].Wp; e.b2 = ctx->g_enc[1].bias;
            e.n_img = c; e.H0 = e.W0 = hw[0]; e.H1 = e.W1 = hw[1]; e.H2 = e.W2 = hw[2]; e.live = live;
            ProfSpan span(ctx, PROF_ENC, st);
            sep12 = launch_conv_e12(e, st);
            if (sep12) span.cancel();
        }
        if (sep12) {
            if (conv_e(1, o4c, c1, ctx->g_enc1p, ctx->g_enc[0].bias, hw[0], hw[1])) {
                // k_conv_g contracts 8 input channels per tap: widen the image first (this path: option enc_tiled = 0)
                if (!o8w) o8w = ctx->allocT<float>(p.o8w);
                if (!o8w) return 1;
                launch_nhwc4_to_8(o4c, o8w, (long)c * hw[0] * hw[0], st);
                conv_g(ctx, PROF_ENC, ctx->g_enc[0], o8w, c1, c, hw[0], 8, hw[1], 32, 0, RowMask{}, st);
            }
            if (conv_e(2, c1, c2, ctx->g_enc[1].Wp, ctx->g_enc[1].bias, hw[1], hw[2]))
                conv_g(ctx, PROF_ENC, ctx->g_enc[1], c1, c2, c, hw[1], 32, hw[2], 32, 0, RowMask{}, st);
        }
        conv_g(ctx, PROF_ENC, ctx->g_enc[2], c2, c3, c, hw[2], 32, hw[3], 64, 0, RowMask{}, st);
        conv_g(ctx, PROF_ENC, ctx->g_enc[3], c3, c4, c, hw[3], 64, hw[4], 64, 0, RowMask{}, st);
        dense_head(ctx, true, c4, flat, enc + (size_t)m0 * 32, 32, hA, hB, c, nc, m0, st);
    }
    return 0;
}

}  // namespace

// ---- what other host files call (engine.h) -----------------------------------------------------------
// the noise addressing of one network pass: key words, rows per group and this rank's row offset, the group -> (pass, sample, stage) map,
// and optionally the row identities / liveness mask of an efe_rows call (one entry = div rows)
NoiseCfg make_noise(uint32_t k0, uint32_t k1, int rows_per_group, uint32_t row_offset, GroupMap gm, const int32_t* ids, int div, const uint8_t* mask) {
    NoiseCfg nc;
    nc.k0 = k0; nc.k1 = k1; nc.rows_per_group = rows_per_group; nc.row_offset = row_offset;
    nc.gm = gm; nc.gm.ids = ids; nc.gm.ids_div = div;
    nc.mask = mask; nc.mask_div = div;
    return nc;
}
// ... of a single-group call over M rows: the caller's seed, stage and row offset, one (pass, sample)
NoiseCfg pass_noise(const efe_noise* nz, uint32_t pass, uint32_t sample, int M) {
    return make_noise((uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), M, nz->row_offset, GroupMap{1, 1, {pass, 0, 0}, nz->stage, sample});
}

// the plans that a second file reads (their structs: engine.h), and the sums efe_rollout_scratch_bytes adds up
RolloutPlan rollout_plan(const efe_ctx* ctx, int64_t M) { return {(size_t)M * 32, (size_t)M * 16, ctx->generic ? (size_t)M * ctx->img_store : 0}; }
size_t plan_bytes(const efe_ctx* c, const RolloutPlan& p) { return arena_bytes(c, {p.enc0, p.x, p.o8}); }
DecTailPlan dec_tail_plan(int64_t M, bool own_y1, bool own_y2, bool own_y3, bool own_po) {
    const size_t C = (size_t)std::min<int64_t>(DEC_TAIL_ROWS, M);
    const int G = dec_tail_slabs((int)std::min<int64_t>(M, DEC_TAIL_SLABS));
    return {(int)C, G, own_y1 ? C * DEC_TAIL_Y1 : 0, own_y2 ? C * DEC_TAIL_Y2 : 0, own_y3 ? C * DEC_TAIL_Y3 : 0, own_po ? C * 4096 : 0,
            C * 4096, C * DEC_TAIL_Y3, C * DEC_TAIL_Y2, C * DEC_TAIL_Y1, G > 1 ? (size_t)G * DEC_TAIL_P : 0};
}
DecHeadPlan dec_head_plan(int64_t M, bool own_h1, bool own_h2, bool own_h3, bool own_h4) {
    const size_t C = (size_t)std::min<int64_t>(DEC_TAIL_ROWS, M);
    const int G = dec_head_slabs((int)std::min<int64_t>(M, 16 * DEC_HEAD_SLABS));
    return {(int)C, G, own_h1 ? C * 256 : 0, own_h2 ? C * 256 : 0, own_h3 ? C * 256 : 0, own_h4 ? C * DEC_TAIL_Y1 : 0, C * DEC_TAIL_Y1,
            (size_t)DEC_HEAD_SEGS * C * 256, G > 1 ? (size_t)G * DEC_HEAD_SMALL_P : 0};
}
size_t encoder_bytes(const efe_ctx* ctx, int64_t N) { return ctx->generic ? plan_bytes(ctx, enc_g_plan(ctx, N)) : plan_bytes(ctx, enc_plan(ctx, N)); }
size_t core_bytes(const efe_ctx* ctx, int64_t R, int64_t D, int64_t S, bool own_terms) {
    return plan_bytes(ctx, core_plan(ctx, R, D, S, true, own_terms)) + (size_t)D * plan_bytes(ctx, mid_plan(ctx, 2 * S * R))
         + decoder_bytes(ctx, D * 3 * S * R) + encoder_bytes(ctx, D * S * R);
}

// ModelMid.ps_net over M = groups*R rows; X is [R][16], every group reads the same rows (x_mod).
int run_mid(efe_ctx* ctx, const float* X, int x_mod, int M, float* tr /*[M][32]*/, const NoiseCfg& nc, hipStream_t st) {
    ctx->last_macs += (int64_t)M * ctx->mac_trans;
    if (!ctx->mid_unfused) {           // one launch for the four layers, activations in LDS (fused.hip)
        TransFusedArgs a{};
        a.W = ctx->mid16; a.X = X; a.tr = tr; a.M = M; a.x_mod = x_mod;
        set_keys(a, nc, 0);
        ProfSpan span(ctx, PROF_MID, st);
        launch_trans_fused(a, st);
        return 0;
    }
    const MidPlan p = mid_plan(ctx, M);
    float* h1 = ctx->allocT<float>(p.h1);
    float* h2 = ctx->allocT<float>(p.h2);
    if (!h1 || !h2) return 1;
    fc(ctx, PROF_MID, ctx->mid[0], X, 16, x_mod, h1, 512, M, true, true, TAG_MID + 0, nc, 0, st);
    fc(ctx, PROF_MID, ctx->mid[1], h1, 512, 0, h2, 512, M, true, true, TAG_MID + 1, nc, 0, st);
    fc(ctx, PROF_MID, ctx->mid[2], h2, 512, 0, h1, 512, M, true, true, TAG_MID + 2, nc, 0, st);
    fc(ctx, PROF_MID, ctx->mid[3], h1, 512, 0, tr, 32, M, false, false, 0, nc, 0, st);
    return 0;
}

// ModelDown.po_net over N rows ([group][row] batch): the three small dense layers run once over all rows, then per
// chunk: dense 256->16384 (+dropout) -> k_dec_a (two transposed convs through LDS) -> k_dec_b (third transposed conv,
// final conv, sigmoid and the per-image reduction, all on chip); under dec_fuse_ab the last two as one launch, k_dec_ab (dec_fused).
int run_decoder(efe_ctx* ctx, const float* dec_in /*[N][16]*/, int N, const NoiseCfg& nc, int reward0, int store0,
                float* val /*[N], or [N][4] quarter sums when dec_split(ctx, N)*/, float* po_store, hipStream_t st) {
    if (ctx->generic) return run_decoder_g(ctx, dec_in, N, nc, reward0, store0, val, po_store, st);
    // po_net.19.bias goes to k_dec_b4 by value: after a device-side optimiser step (efe_train_down / efe_down_adam_step) the host scalar is
    // stale, and the first decoder pass behind the step fetches the 4 bytes on its own stream, once
    if (ctx->dec_bf_stale) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            return ctx->fail("decoder: the first pass after an optimiser step of ModelDown synchronises its stream once and cannot be captured");
        if (hipMemcpyAsync(&ctx->dec_bf, ctx->down_master + DOWN_P - 1, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return ctx->fail("decoder: fetching po_net.19.bias after an optimiser step failed");
        ctx->dec_bf_stale = false;
    }
    const DecPlan p = dec_plan(ctx, N);
    const bool split = p.split;
    // mfma_f16x2 marks a row / image whose activation overflowed fp16 with +inf, and only its own split kernels turn that into a NaN
    // sum: an exact-fp32 consumer (k_dec_a_s / k_dec_a / k_dec_b4) can make a finite wrong image of it (inf - inf = NaN, and a ReLU
    // maps a negative-signed NaN or -inf to 0).  So under that mode the chain is split from k_fc4_b3 to k_dec_b_b3 or not at all: small
    // launches keep k_fc4 too, and ConvT3 always runs on k_dec_b_b3 (b3_convt3 = 0 applies to mfma_bf16x3, which cannot overflow).
    const bool f16 = ctx->mfma_bf16x3 == 2;
    const bool fc4_16 = !(f16 && split), ct3_16 = ctx->b3_convt3 || f16;
    const int C = p.C;
    float* hA = ctx->allocT<float>(p.hA);
    float* hB = ctx->allocT<float>(p.hB);
    float* x4 = ctx->allocT<float>(p.x4);
    float* y2 = ctx->allocT<float>(p.y2);
    if (!hA || !hB || !x4 || !y2) return 1;
    ctx->last_macs += (int64_t)N * ctx->mac_dec;
    dense_head(ctx, false, dec_in, 16, hA, 256, hA, hB, N, nc, 0, st);
    int* queues = ctx->allocT<int>(p.queues);
    if (!queues) return 1;
    if (!split && hipMemsetAsync(queues, 0, p.queues * sizeof(int), st) != hipSuccess) return ctx->fail("hipMemsetAsync failed");      // (k_dec_a_s takes no tickets)
    for (int m0 = 0; m0 < N; m0 += C) {
        const int c = std::min(C, N - m0);
        fc(ctx, PROF_DEC_FC4, ctx->dec_fc[3], hA + (size_t)m0 * 256, 256, 0, x4, 16384, c, true, true, TAG_DEC + 3, nc, m0, st, fc4_16);
        if (p.fused) {       // one launch: y2 stays in the workgroups' slots
            DecABArgs ab{};
            DecAArgs& da = ab.a; DecBArgs& db = ab.b;
            da.x4 = x4; da.y2 = y2; da.w1 = ctx->dec_ct[0].Wp; da.b1 = ctx->dec_ct[0].bias; da.w2 = ctx->dec_ct[1].Wp;
            da.b2 = ctx->dec_ct[1].bias; da.rows = c; da.live = live_of(nc, m0); da.queue = queues + m0 / C; da.parts = 1;
            db.y2 = y2; db.w3 = ctx->dec_ct[2].Wp; db.b3 = ctx->dec_ct[2].bias; db.w4 = ctx->dec_wf; db.b4 = ctx->dec_bf;
            db.rows = c; db.live = da.live; db.m0 = m0; db.rows_per_group = nc.rows_per_group; db.gm = nc.gm; db.reward0 = reward0; db.store0 = store0;
            db.val = val; db.parts = 1; db.valq = nullptr; db.po = po_store; db.reward_intent = (int)ctx->reward_intent;
            ProfSpan span(ctx, PROF_CT2, st);      // (never timed: see dec_fused)
            launch_dec_ab(ab, (int)ctx->dec_ab_grid, st);
            continue;
        }
        DecAArgs da{};
        da.x4 = x4; da.y2 = y2; da.w1 = ctx->dec_ct[0].Wp; da.b1 = ctx->dec_ct[0].bias; da.w2 = ctx->dec_ct[1].Wp;
        da.b2 = ctx->dec_ct[1].bias; da.rows = c; da.live = live_of(nc, m0); da.queue = queues + m0 / C; da.parts = split ? 8 : 1;
        {
            ProfSpan span(ctx, PROF_CT2, st);
            if (ctx->mfma_bf16x3 && ctx->ct_b3[0] && !split) {      // opt-in experiment
                da.w1b3 = ctx->ct_b3[0]; da.w2b3 = ctx->ct_b3[1]; da.split = (int)ctx->mfma_bf16x3;
                da.w1s = ctx->s_ct[0]; da.w1s_inv = 1.0f / ctx->s_ct[0]; da.w2s = ctx->s_ct[1]; da.w2s_inv = 1.0f / ctx->s_ct[1];
                launch_dec_a_b3(da, st);
            }
            else launch_dec_a(da, st);
        }
        DecBArgs db{};
        db.y2 = y2; db.w3 = ctx->dec_ct[2].Wp; db.b3 = ctx->dec_ct[2].bias; db.w4 = ctx->dec_wf; db.b4 = ctx->dec_bf;
        db.rows = c; db.live = live_of(nc, m0); db.m0 = m0; db.rows_per_group = nc.rows_per_group; db.gm = nc.gm; db.reward0 = reward0; db.store0 = store0;
        db.val = val; db.parts = split ? 4 : 1; db.valq = split ? val : nullptr; db.po = po_store; db.reward_intent = (int)ctx->reward_intent;
        ProfSpan span(ctx, PROF_CT3, st);
        if (ctx->mfma_bf16x3 && ct3_16 && ctx->ct3_b3 && !split) {      // opt-in experiment
            db.w3b3 = ctx->ct3_b3; db.split = (int)ctx->mfma_bf16x3; db.w3s = ctx->s_ct3; db.w3s_inv = 1.0f / ctx->s_ct3;
            launch_dec_b_b3(db, st);
        }
        else launch_dec_b(db, st);
    }
    return 0;
}

// ModelDown.qs_net over N rows; o is [N][4096]; out enc [N][32] (mean 0..9, logvar 10..19).
int run_encoder(efe_ctx* ctx, const float* o, int N, const NoiseCfg& nc, float* enc, hipStream_t st) {
    if (ctx->generic) return run_encoder_g(ctx, o, N, nc, enc, st);
    const EncPlan p = enc_plan(ctx, N);
    const int C = p.C;
    float* c4 = ctx->allocT<float>(p.c4);
    float* hA = ctx->allocT<float>(p.hA);
    float* hB = ctx->allocT<float>(p.hB);
    if (!c4 || !hA || !hB) return 1;
    ctx->last_macs += (int64_t)N * ctx->mac_enc;
    for (int m0 = 0; m0 < N; m0 += C) {
        const int c = std::min(C, N - m0);
        EncArgs ea{};
        ea.o = o + (size_t)m0 * 4096; ea.out = c4; ea.w1 = ctx->enc_w1; ea.b1 = ctx->enc_b1;
        ea.w2 = ctx->enc_conv[0].Wp; ea.b2 = ctx->enc_conv[0].bias; ea.w3 = ctx->enc_conv[1].Wp; ea.b3 = ctx->enc_conv[1].bias;
        ea.w4 = ctx->enc_conv[2].Wp; ea.b4 = ctx->enc_conv[2].bias; ea.rows = c; ea.live = live_of(nc, m0);
        {
            ProfSpan span(ctx, PROF_ENC, st);
            launch_enc_trunk(ea, st);
        }
        dense_head(ctx, true, c4, 576, enc + (size_t)m0 * 32, 32, hA, hB, c, nc, m0, st);
    }
    return 0;
}

int run_habit(efe_ctx* ctx, const float* s16 /*[M][16]*/, int M, float* l32 /*[M][32]*/, hipStream_t st) {
    float* h1 = ctx->allocT<float>((size_t)M * 128);
    float* h2 = ctx->allocT<float>((size_t)M * 128);
    if (!h1 || !h2) return 1;
    NoiseCfg nc;
    fc(ctx, PROF_OTHER, ctx->top[0], s16, 16, 0, h1, 128, M, true, false, 0, nc, 0, st);
    fc(ctx, PROF_OTHER, ctx->top[1], h1, 128, 0, h2, 128, M, true, false, 0, nc, 0, st);
    fc(ctx, PROF_OTHER, ctx->top[2], h2, 128, 0, l32, 32, M, false, false, 0, nc, 0, st);
    ctx->last_macs += (int64_t)M * ctx->mac_habit;
    return 0;
}

// calculate_G for D chained stages (torchmodel.py:236-243, 270-300)
int run_core(efe_ctx* ctx, const CoreIO& io, hipStream_t st) {
    const int R = io.R, D = io.D, S = io.S;
    const CorePlan plan = core_plan(ctx, R, D, S, !io.pre_tr, !io.terms);
    float* tr_all = io.pre_tr ? io.pre_tr : ctx->allocT<float>(plan.tr_all);
    float* dec_in = ctx->allocT<float>(plan.dec_in);
    float* xbuf = ctx->allocT<float>(plan.xbuf);
    float* val = ctx->allocT<float>(plan.val);
    float* po_store = ctx->allocT<float>(plan.po_store);
    float* enc = ctx->allocT<float>(plan.enc);
    float* terms_tmp = io.terms ? nullptr : ctx->allocT<float>(plan.terms_tmp);
    if (!tr_all || !dec_in || !xbuf || !val || !po_store || !enc) return 1;
    // the noise of a pass over the R logical rows: the call's keys and row identities, the pass's group map
    auto noise = [&](const GroupMap& gm, const uint8_t* mask) { return make_noise(io.k0, io.k1, R, io.row_offset, gm, io.ids, io.mask_div, mask); };

    const float* x = io.x0;
    for (int t = 0; t < D; ++t) {
        float* tr = tr_all + (size_t)t * 2 * S * R * 32;
        if (io.pre_tr) {
            // trajectory mode behind k_sim_chain: it has written both groups
        } else if (io.given_mean) {
            // trajectory mode: group T1 is supplied, only the loop-2 transition runs
            launch_fill_tr(io.given_mean, io.given_logvar, tr, R, st);
            if (run_mid(ctx, x, R, R, tr + (size_t)R * 32, noise(GroupMap{1, 1, {PASS_T2, 0, 0}, io.stage0 + (uint32_t)t, 0}, nullptr), st)) return 1;
        } else {
            if (run_mid(ctx, x, R, 2 * S * R, tr, noise(GroupMap{2 * S, S, {PASS_T1, PASS_T2, 0}, io.stage0 + (uint32_t)t, 0}, nullptr), st)) return 1;
        }
        TransPostArgs p{};
        p.tr = tr; p.x = x; p.eps_inj = io.eps ? io.eps + (size_t)t * 3 * S * R * 10 : nullptr;
        p.given_ps1 = io.given_ps1;
        p.dec_in = dec_in + (size_t)t * 3 * S * R * 16;
        float* nx = xbuf + (size_t)(t & 1) * R * 16;
        p.next_x = (t + 1 < D) ? nx : nullptr;
        p.ps1_last = (t + 1 == D) ? io.ps1 : nullptr;
        p.ps1_mean_last = (t + 1 == D) ? io.ps1_mean : nullptr;
        p.S = S; p.R = R; p.mean_mode = io.mean_mode; p.carry_mean = io.carry_mean;
        p.k0 = io.k0; p.k1 = io.k1; p.stage = io.stage0 + t; p.row_offset = io.row_offset; p.pi_dim = ctx->pi_dim;
        p.ids = io.ids; p.ids_div = io.mask_div;
        launch_trans_post(p, st);
        x = nx;
    }
    // one batched decoder pass over D x 3S groups, one batched encoder pass over the D x S loop-1 images
    if (run_decoder(ctx, dec_in, D * 3 * S * R, noise(GroupMap{3 * S, S, {PASS_D1, PASS_D2A, PASS_D2B}, io.stage0, 0}, io.mask), 1, 1, val, po_store, st)) return 1;
    if (run_encoder(ctx, po_store, D * S * R, noise(GroupMap{S, S, {PASS_E1, 0, 0}, io.stage0, 0}, io.mask), enc, st)) return 1;
    TermsArgs ta{};
    ta.val = val; ta.valq = plan.vsplit ? val : nullptr; ta.tr = tr_all; ta.enc = enc; ta.D = D; ta.S = S; ta.R = R;
    // term0 of an image = 10 * mean over the pixels that count (torchmodel.py:212: all 4096, or the 192 bar pixels of the
    // upstream-intent variant); the generic geometries use the sum form of the reference's resolution-32 branch (torchmodel.py:214)
    ta.reward_div = ctx->generic ? 0.0f : (ctx->reward_intent ? 192.0f : 4096.0f);
    ta.G = io.G; ta.terms = io.terms ? io.terms : terms_tmp; ta.t2parts = io.t2parts;
    launch_terms(ta, st);
    if (io.po1) {
        const float* last = po_store + ((size_t)(D - 1) * S + (S - 1)) * R * ctx->img_store;
        if (ctx->generic) launch_to_nchw(last, io.po1, R, ctx->res * ctx->res, ctx->chan, st);
        else if (hipMemcpyAsync(io.po1, last, (size_t)R * 4096 * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return ctx->fail("po1 copy failed");
    }
    return 0;
}

}  // namespace host
}  // namespace efe
