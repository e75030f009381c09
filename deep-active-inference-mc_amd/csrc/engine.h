// What the host files of the engine (engine_*.hip) share: the context, the scope of one C ABI call, and the declarations of the few
// helpers that cross a file boundary.  Everything else lives in the anonymous namespace of the one file that uses it.
//   engine_ctx.hip      the registry of live contexts; lifecycle, options, profiling, scratch management
//   engine_weights.hip  weight packing, the training tables, efe_set_weight / efe_commit_weights
//   engine_forward.hip  launch helpers, scratch plans, the forward runners (run_mid ... run_core)
//   engine_efe.hip      network-level and EFE-level entry points
//   engine_control.hip  environment, agent and MCTS entry points
//   engine_loss.hip     the training-side free energy, the epoch report (efe_eval_stats)
//   engine_train.hip    gradients, optimiser steps, efe_train_step
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/efe_engine.h"
#include "ctx_registry.h"
#include "kernels.h"

using namespace efe;

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { return ctx->fail(std::string(#x) + ": " + hipGetErrorString(e_)); } } while (0)

namespace efe {
namespace host {

constexpr int S_DIM = 10;
constexpr int64_t MAC_TRANS = 541696, MAC_DEC = 43256320, MAC_ENC = 3868960, MAC_HABIT = 18176;
constexpr size_t SCRATCH_HEADROOM = (size_t)1 << 20;      // efe_rollout_scratch_bytes reports this much more than the plans add up to

enum ProfClass { PROF_MID = 0, PROF_DEC_FC = 1, PROF_DEC_FC4 = 2, PROF_CT1 = 3, PROF_CT2 = 4, PROF_CT3 = 5, PROF_FINAL = 6,
                 PROF_ENC = 7, PROF_OTHER = 8, PROF_NCLS = 9 };

struct HostTensor { std::vector<float> data; std::vector<int64_t> shape; };

struct Layer {
    float* Wp = nullptr; float* bias = nullptr;
    int cin = 0;      // padded K per tap
    int cout = 0; int mtiles = 0; int ntaps = 1;
};

struct LayerSpec { const char* key; int out, in; };       // one layer of a network as the weight tables list it (see top_layer / mid_layer)
struct TrainPart {
    float* master = nullptr; TrainNet* net_dev = nullptr; TrainNet net{};
    bool dirty = false;
    int nl = 0; LayerSpec (*layer)(int, int) = nullptr;      // the part's layers (keys of `raw`)
    const char* prefix = "";                                   // "top." / "mid.": the keys efe_set_weight must not revert
};

struct Arena {
    std::vector<std::pair<char*, size_t>> blocks;
    size_t cur = 0, off = 0, used_total = 0;
    void reset() { cur = 0; off = 0; used_total = 0; }
    // the bump position, to put back once a chunk's scratch is done with (the blocks stay)
    struct Mark { size_t cur, off, used_total; };
    Mark mark() const { return {cur, off, used_total}; }
    void rewind(const Mark& m) { cur = m.cur; off = m.off; used_total = m.used_total; }
    size_t capacity() const { size_t n = 0; for (auto& b : blocks) n += b.second; return n; }
};

}  // namespace host
}  // namespace efe

using namespace efe::host;

struct efe_ctx {
    int device = 0;
    std::string err;
    std::map<std::string, HostTensor> raw;
    bool committed = false;
    Layer top[3], mid[4], enc_conv[3], enc_fc[4], dec_fc[4], dec_ct[3];
    // geometry: the reference's Dynamic-dSprites configuration (pi 4, 1 x 64 x 64) runs on the fused kernels; any other
    // (pi_dim, channels, resolution) runs the generic layer-by-layer convolution path (generic.hip; SURVEY 8a-13, parity unpinned)
    int pi_dim = 4, chan = 1, res = 64;
    bool generic = false;
    bool last_s1 = false;           // resolution 32: the reference's own variant (torchmodel.py:77-80, last_strides = 1): decoder base res/2, third ConvT stride 1
    int base = 16, enc_hw[5] = {64, 31, 15, 7, 3};
    size_t img_store = 4096;        // floats per stored D1 image: C*H*W NCHW (dSprites, C = 1) or H*W*4 NHWC4 (generic)
    Layer g_fc4, g_ct[3], g_enc[4];
    float* g_wf = nullptr; float g_bf[4] = {0.f, 0.f, 0.f, 0.f};
    float* g_enc1p = nullptr;       // first encoder conv for k_conv_e: [9 taps][64 lanes][2] = W[co][h][tap], W[co][2 + h][tap]
    int64_t mac_dec = 43256320, mac_enc = 3868960, mac_trans = 541696, mac_habit = 18176;
    MlpW dec16{}, enc16{};         // decoder / encoder dense heads packed the same way (k_head)
    int enc16_kc0 = 0;
    int64_t head_unfused = 0;      // option: 1 = layer-by-layer k_dense heads (A/B experiments)
    MlpW mid16{}, top16{};         // the same transition / habit weights packed for the fused 16x16x4 kernels (fused.hip)
    // training (train.hip), per trainable part (habit net "top", transition net "ps_net"): the fp32 master copy (flat, the reference's
    // parameters() order), its layer table on the host and on the device, and whether an optimiser step has made the device copy newer
    // than `raw`
    TrainPart top_train, mid_train;
    int64_t mid_unfused = 0;       // option: 1 = layer-by-layer k_dense transition (A/B experiments)
    float *enc_w1 = nullptr, *enc_b1 = nullptr, *dec_wf = nullptr;
    float dec_bf = 0.f;
    float* dec_raw = nullptr;      // the whole po_net unpacked, flat in parameters() order (kernels.h DH_*, then DT_*): train_dec_head.hip reads it
    float* dect_raw = nullptr;     // its tail po_net.13 / .15 / .17 / .19 (= dec_raw + DEC_HEAD_P): train_dec.hip reads it
    float* dect_raw_g = nullptr;   // the same tail at ANY geometry, [92 320 + 289 chan] (DecTailGeo): train_dec_g.hip reads it.  = dect_raw at 1 x 64 x 64,
                                   // else the tail of down_master_g (either way it follows ModelDown's optimiser steps)
    float* dec_raw_g = nullptr;    // the whole po_net at ANY geometry, [134 400 + 257 * 64 base^2] (DecHeadGeo) then the tail: train_dec_head_g.hip
                                   // reads it.  dect_raw_g = dec_raw_g + the head's size; = dec_raw at 1 x 64 x 64, else down_master_g + EncGeo::P()
    float* enc_raw = nullptr;      // the whole qs_net unpacked, flat in parameters() order (kernels.h EQ_*): train_enc.hip reads it
    float* enc_raw_g = nullptr;    // the same at ANY geometry, [201 684 + 288 chan + 256 K] (EncGeo): train_enc_g.hip reads it.  = enc_raw at 1 x 64 x 64,
                                   // else down_master_g (either way it follows ModelDown's optimiser steps); enc_raw stays null there
    // ModelDown's master copy at 1 x 64 x 64 (owned: it outlives a re-commit, as TrainPart::master): [DOWN_P], qs_net then po_net, so
    // enc_raw = down_master and dec_raw = down_master + ENC_P.  An optimiser step (train_down.hip) writes it and rebuilds every packed form
    // of the table down_repack (device; one entry per packed buffer of pack_heads / pack_encoder / pack_decoder, built at commit).
    // down_dirty: the device copy is newer than raw["down.*"] (refresh_down_host).  dec_bf_stale: and newer than the host scalar dec_bf.
    float* down_master = nullptr;
    RepackDesc* down_repack = nullptr; int down_repack_n = 0, down_repack_blocks = 0;
    bool down_dirty = false, dec_bf_stale = false;
    // The same on a generic context (every other geometry): [down_g_count()], qs_net (EncGeo) then po_net (DecHeadGeo, then the tail), owned,
    // allocated at the first commit and refilled by a re-commit; enc_raw_g / dec_raw_g / dect_raw_g are spans of it.  An optimiser step
    // (efe_train_down_g / efe_down_adam_step_g) writes it and rebuilds every packed form of the table down_repack_g (train_down_g.hip;
    // built at every commit from that commit's buffers).  g_bf_stale: the master copy is newer than the host floats g_bf.
    float* down_master_g = nullptr;
    RepackDesc* down_repack_g = nullptr; int down_repack_g_n = 0, down_repack_g_blocks = 0;
    bool g_bf_stale = false;
    float* zeros = nullptr;
    std::vector<void*> owned;      // lives as long as the context
    std::vector<void*> wbufs;      // packed weights of the current commit (freed by the next one)
    Arena arena;
    // One scratch arena per context: calls are serialised by `mu` (host threads) and ordered across streams by `done_ev`
    // (a call on a different stream than the previous one first waits for that call's last kernel), so the arena reset at the
    // start of a call never races with work still in flight.  `mu` and `dead` belong to the registry's protocol (ctx_registry.h).
    std::mutex mu; bool dead = false;
    hipStream_t last_stream = nullptr;
    bool have_last = false;
    hipEvent_t done_ev = nullptr;
    size_t high_water = 0;         // largest arena use of any call so far (bytes)
    int64_t arena_grows = 0;       // number of hipMalloc calls the arena has made
    int64_t dec_chunk = 32768, enc_chunk = 32768, poison = -1, trace = 0, dec_chunk_g = 16384;
    int64_t dec_budget_g = (int64_t)28 << 30;
    // generic decoder: images per launch group = min(dec_chunk, dec_chunk_g, dec_budget_g / activation bytes per image), so the scratch
    // block of a launch group is bounded in BYTES whatever the resolution (0.68 MB of layer activations per image at 84 x 84 on the
    // fused path, 1.6 MB with the final layer unfused); poison / trace: development only
    int64_t arena_align = 256;
    int64_t reward_intent = 0;     // option "reward_upstream_intent": 1 = the reward target the upstream NHWC code means (kernels.h reward_term), 0 = the shipped port's
    int64_t ct_fuse12 = 1;         // generic path, decoder ConvT layers 1 and 2: 1 = one kernel, layer 1's output kept in LDS (k_convt_12); 0 = one launch per layer
    int64_t enc_tiled = 2;         // generic path, encoder layers 1 and 2: 2 = one kernel, conv1 kept in LDS (k_conv_e12); 1 = LDS-tiled, one launch per layer
                                   // (k_conv_e); 0 = k_conv_g for every layer (A/B, parity of the fallbacks)
    int64_t dec_split = 1;         // dSprites path: decoder launches of <= 128 images run k_dec_b4 with four workgroups per image (0 = never: A/B)
    int64_t dec_fuse_ab = 1;       // dSprites path, fp32 launches of > 128 images: 1 = k_dec_a and k_dec_b4 as one persistent launch, k_dec_ab, y2 in one 256 KiB slot
                                   // per workgroup (engine_forward.hip dec_fused); 0 = two launches, y2 for every image of a launch group
    int64_t dec_ab_grid = 0;       // cap of k_dec_ab's grid (0 = min(512, images)): lets a small launch give every workgroup several images (tests)
    int64_t fuse_final_g = 1;      // generic path: last two decoder layers in one kernel (k_dec_bg); 0 = separate launches (A/B, parity tests of k_final_g)
    // OPT-IN EXPERIMENTS (bf16x3.hip): the decoder's Linear(256, 16384) and three large ConvTranspose2d layers on the 16-bit matrix pipe with
    // split operands.  mfma_bf16x3 holds the MODE: 0 = off (exact fp32, the default), 1 = three bf16 planes / six products (option
    // "mfma_bf16x3"), 2 = two fp16 planes / three products (option "mfma_f16x2").  The planes below are packed for `split_packed`.
    int64_t mfma_bf16x3 = 0;
    int split_packed = 0;
    uint16_t* fc4_b3 = nullptr;    // po_net.9's packed planes (part of wbufs)
    uint16_t* ct_b3[2] = {nullptr, nullptr};      // po_net.13 / .15 (k_dec_a's layers) as planes
    uint16_t* ct3_b3 = nullptr;                   // po_net.17 (ConvT3, k_dec_b_b3) as planes
    float s_fc4 = 1.f, s_ct[2] = {1.f, 1.f}, s_ct3 = 1.f;      // fp16 split: the power of two each layer's weights were scaled by
    int64_t b3_convt3 = 1;                        // mfma_bf16x3: ConvT3 on the bf16 pipe too (0 = the fp32 k_dec_b4 behind the two bf16 kernels, round 5's form)
    bool arch_gfx950 = false;      // hipDeviceProp_t.gcnArchName starts with gfx950 (checked at creation)
    int64_t sim_split = 1;         // simulations of <= 16 episodes: the chain kernel on eight workgroups per 8 episodes (k_sim_chain<8>); 0 = one workgroup (A/B, bit-identical)
    bool sim_sync_dirty = false;   // the last split launch's call did not complete on the host: zero sim_sync before the next one
    double* mi_ws = nullptr;       // efe_eval_mi's column statistics and per-slice partial sums [EVAL_MI_WS], then its digamma table [EVAL_MI_PSI] (owned)
    float* sim_xch = nullptr; int* sim_sync = nullptr;      // its exchange buffer and arrival counters / sticky timeout flag (owned; zeroed at creation, and on the stream when sim_sync_dirty; otherwise, after an in-kernel timeout too, the kernel's epilogue re-arms them)
    int64_t check_rows = 0;        // development: range-check efe_rows.ids on the host before every _rows call
    int64_t last_macs = 0;
    // optional per-kernel-class timing with HIP events on the launch stream (bench.py roofline)
    unsigned prof = 0;        // bitmask of ProfClass values to time
    int cls = PROF_OTHER;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> ev_spans;
    hipEvent_t ev_get() {
        if (ev_used == ev_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); ev_pool.push_back(e); }
        return ev_pool[ev_used++];
    }
    int trace_n = 0;
    hipEvent_t prof_begin(hipStream_t st) {
        if (trace) { (void)hipStreamSynchronize(st); fprintf(stderr, "[efe trace] launch %d class %d ...\n", ++trace_n, cls); fflush(stderr); return (hipEvent_t)1; }
        if (!(prof & (1u << cls))) return nullptr;
        hipEvent_t a = ev_get(); (void)hipEventRecord(a, st); return a;
    }
    void prof_end(hipEvent_t a, hipStream_t st) {
        if (trace) { hipError_t e = hipStreamSynchronize(st); fprintf(stderr, "[efe trace] launch %d done: %s\n", trace_n, hipGetErrorString(e)); fflush(stderr); return; }
        if (!a) return;
        hipEvent_t b = ev_get(); (void)hipEventRecord(b, st);
        ev_spans.push_back({cls, {a, b}});
    }

    std::string pending;      // error raised inside a launch helper, reported by finish()
    int fail(const std::string& m) { err = m; return 1; }

    // bump allocator over a list of device blocks; grows (synchronously) on first use at a new size
    size_t al(size_t bytes) const { return (bytes + (size_t)arena_align - 1) / (size_t)arena_align * (size_t)arena_align; }
    void* alloc(size_t bytes) {
        bytes = al(bytes);
        while (true) {
            if (arena.cur < arena.blocks.size()) {
                auto& b = arena.blocks[arena.cur];
                if (arena.off + bytes <= b.second) {
                    void* p = b.first + arena.off; arena.off += bytes; arena.used_total += bytes;
                    if (arena.used_total > high_water) high_water = arena.used_total;
                    return p;
                }
                arena.cur++; arena.off = 0;
                continue;
            }
            size_t sz = std::max(bytes, (size_t)256 << 20);
            char* p = nullptr;
            if (hipMalloc((void**)&p, sz) != hipSuccess) { err = "arena hipMalloc failed"; return nullptr; }
            arena.blocks.push_back({p, sz});
            ++arena_grows;
        }
    }
    template <class T> T* allocT(size_t n) { return reinterpret_cast<T*>(alloc(n * sizeof(T))); }
};

namespace efe {
namespace host {

constexpr int TOP_NL = 3, MID_NL = 4;      // layers of the habit net / the transition net (top_layer / mid_layer)

struct NoiseCfg {
    uint32_t k0 = 0, k1 = 0;
    GroupMap gm{1, 1, {0, 0, 0}, 0, 0};
    int rows_per_group = 1;
    uint32_t row_offset = 0;
    const uint8_t* mask = nullptr;      // liveness of the logical rows (efe_rows.mask), entry = row / mask_div
    int mask_div = 1;
};

// The profiling span of one launch: the launches of its scope count under class `cls` (efe_prof_read), between two events on the stream when
// that class is being timed.  The end of the scope closes the span and puts the class back; cancel() = nothing was launched, record no span.
struct ProfSpan {
    efe_ctx* const ctx; const hipStream_t st; const int prev; hipEvent_t e0;
    ProfSpan(efe_ctx* c, int cls, hipStream_t s) : ctx(c), st(s), prev(c->cls) { c->cls = cls; e0 = c->prof_begin(s); }
    void cancel() { e0 = nullptr; }
    ~ProfSpan() { ctx->prof_end(e0, st); ctx->cls = prev; }
};

struct CoreIO {
    const float* x0;          // [R][16] = [pi | s0 | 0 0]
    int R, D, S, mean_mode, carry_mean;
    uint32_t k0, k1, stage0, row_offset;
    const float* eps;         // nullable, per stage [3S][R][10]
    const uint8_t* mask = nullptr; int mask_div = 1;        // liveness of the R logical rows (efe_rows.mask): entry slot = row / mask_div
    const int32_t* ids = nullptr;                           // entry slot -> entry id (efe_rows.ids): noise keys and the mask follow the id
    // trajectory mode (D == 1, S == 1): T1 is given
    const float* given_ps1 = nullptr; const float* given_mean = nullptr; const float* given_logvar = nullptr;
    float* pre_tr = nullptr;  // trajectory mode: both transition groups [2][R][32] already computed (k_sim_chain)
    float *G = nullptr, *terms = nullptr, *ps1 = nullptr, *ps1_mean = nullptr, *po1 = nullptr, *t2parts = nullptr;
};

// the root of efe_rollout: the encoded observation, the first transition input, and (generic geometry) the observation as NHWC4
struct RolloutPlan { size_t enc0, x, o8; };
// efe_dec_tail_grad (train_dec.hip): the stored activations and the gradients of one row group (C rows; y_l / po exist only when the caller
// gives no output for them), nlogpo1 never (required output), and the partial-gradient slabs (none at G = 1: the gradient itself)
struct DecTailPlan { int C, G; size_t y1, y2, y3, po, g4, g3, g2, g1, slabs; };
// efe_dec_grad (train_dec_head.hip) on top of the tail's plan: the head's stored activations of one row group (those the caller gives no
// output for), d_h4 (gated in place to layer 3's gradient), the 64 segment partials of d_h3, and the slabs of layers 0..2 (none at G = 1)
struct DecHeadPlan { int C, G; size_t h1, h2, h3, h4, dh4, part, slabs; };

// puts the caller's device back on exit if it is not `dev` (< 0: none): a call on a context of GPU 1 must not leave the thread on GPU 1
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) { int cur = -1; if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur; }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// engine_ctx.hip: the one registry of live contexts, and whether `st` is being captured into a hipGraph
CtxRegistry<efe_ctx>& registry();
bool capturing(hipStream_t st);

// The scope of one C ABI call: it admits the handle (ctx->mu held to its end) and puts the caller's device back on every exit.  Modes: host,
// nothing more; device, the context's device made current; scratch, that and a call on the scratch arena on stream `st`: work of the previous
// call still in flight on ANOTHER stream finishes first (same stream: stream order guarantees it), and every exit after that -- success or
// failure, kernels maybe queued -- records done_ev behind `st`'s work, so that the next call, on any stream, can order its arena reuse behind it.
// false: a refused handle (return code 1, efe_last_error explains) or a failed start (its message in ctx->err).
// ordered: scratch's ordering for a call that reads no weights and works in a buffer the context owns (efe_eval_mi: ctx->mi_ws).
enum class Mode { host, device, scratch, ordered };
// what efe_last_error says of a handle that is not live, on this thread: the plain message, or (Call::refused) the one that names the entry
// point which was just handed it; every new call scope puts the plain one back
extern thread_local std::string tl_stale_msg;      // (engine_ctx.hip)
struct Call {
    CtxRegistry<efe_ctx>::Admission adm;
    efe_ctx* const ctx;
    DeviceScope dev;
    hipStream_t st;
    bool ok = false, record = false;
    Call(efe_ctx* c, Mode mode, hipStream_t stream = nullptr)
        : adm(registry().admit(c)), ctx(adm.ctx.get()), dev(ctx ? ctx->device : -1), st(stream) { tl_stale_msg.clear(); ok = ctx && !start(mode); }
    // the return value of an entry point whose scope did not open: 1; a refused handle's message names the entry point
    int refused(const char* who) const {
        if (!ctx) tl_stale_msg = std::string(who) + ": stale or invalid context handle";
        return 1;
    }
    int start(Mode mode) {
        if (mode == Mode::scratch && !ctx->committed) return ctx->fail("weights not committed");
        if (mode != Mode::host && hipSetDevice(ctx->device) != hipSuccess) return ctx->fail("hipSetDevice failed");
        if (mode == Mode::host || mode == Mode::device) return 0;
        if (ctx->have_last && ctx->last_stream != st && !capturing(st) && hipStreamWaitEvent(st, ctx->done_ev, 0) != hipSuccess)
            return ctx->fail("hipStreamWaitEvent failed");
        ctx->arena.reset();
        if (ctx->poison >= 0)                      // development: every call starts on scratch filled with this byte (reads of never-written scratch show up)
            for (auto& b : ctx->arena.blocks)
                if (hipMemsetAsync(b.first, (int)(ctx->poison & 0xff), b.second, st) != hipSuccess) return ctx->fail("poison memset failed");
        ctx->last_macs = 0;
        record = true;
        return 0;
    }
    ~Call() {
        if (record && !capturing(st) && hipEventRecord(ctx->done_ev, st) == hipSuccess) { ctx->last_stream = st; ctx->have_last = true; }
        if (ctx) ctx->pending.clear();             // a launch helper's error belongs to this call, reported or not
    }
    explicit operator bool() const { return ok; }
    // the end of a call that queued kernels: an error raised inside a launch helper, else the last launch error
    int finish() {
        if (!ctx->pending.empty()) return ctx->fail(ctx->pending);
        hipError_t e = hipGetLastError();
        return e == hipSuccess ? 0 : ctx->fail(std::string("kernel launch: ") + hipGetErrorString(e));
    }
};

// ---- engine_weights.hip ------------------------------------------------------------------------------
LayerSpec top_layer(int i, int A);
LayerSpec mid_layer(int i, int A);
int part_param_count(int nl, LayerSpec (*layer)(int, int), int A);
int refresh_down_host(efe_ctx* ctx);
int64_t down_g_count(const efe_ctx* ctx);       // floats of ModelDown at the context's geometry: efe_param_count("down_g")
int pack_fc4_b3(efe_ctx* ctx, int mode);

// ---- engine_forward.hip ------------------------------------------------------------------------------
NoiseCfg make_noise(uint32_t k0, uint32_t k1, int rows_per_group, uint32_t row_offset, GroupMap gm, const int32_t* ids = nullptr, int div = 1,
                    const uint8_t* mask = nullptr);
NoiseCfg pass_noise(const efe_noise* nz, uint32_t pass, uint32_t sample, int M);
RolloutPlan rollout_plan(const efe_ctx* ctx, int64_t M);
size_t plan_bytes(const efe_ctx* c, const RolloutPlan& p);
DecTailPlan dec_tail_plan(int64_t M, bool own_y1, bool own_y2, bool own_y3, bool own_po);
DecHeadPlan dec_head_plan(int64_t M, bool own_h1, bool own_h2, bool own_h3, bool own_h4);
size_t encoder_bytes(const efe_ctx* ctx, int64_t N);
size_t core_bytes(const efe_ctx* ctx, int64_t R, int64_t D, int64_t S, bool own_terms);
int run_mid(efe_ctx* ctx, const float* X, int x_mod, int M, float* tr /*[M][32]*/, const NoiseCfg& nc, hipStream_t st);
int run_decoder(efe_ctx* ctx, const float* dec_in /*[N][16]*/, int N, const NoiseCfg& nc, int reward0, int store0,
                float* val /*[N], or [N][4] quarter sums when the launch is split*/, float* po_store, hipStream_t st);
int run_encoder(efe_ctx* ctx, const float* o, int N, const NoiseCfg& nc, float* enc, hipStream_t st);
int run_habit(efe_ctx* ctx, const float* s16 /*[M][16]*/, int M, float* l32 /*[M][32]*/, hipStream_t st);
int run_core(efe_ctx* ctx, const CoreIO& io, hipStream_t st);

// ---- engine_loss.hip ---------------------------------------------------------------------------------
int fe_params(efe_ctx* ctx, const efe_fe_params* p, bool derived_ok, const char* who);
void fe_omega(FeArgs& a, const efe_fe_params* p);
FeArgs fe_down_args(efe_ctx* ctx, int M, const float* o1, const float* enc, const float* p1_mean, const float* p1_lv, int p1_ld,
                    const efe_fe_params* p, const float* omega, const efe_fe_out* out);

}  // namespace host
}  // namespace efe
