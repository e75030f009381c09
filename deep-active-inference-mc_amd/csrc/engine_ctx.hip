// Host side of the EFE rollout engine: context, weight packing, launch orchestration and the C ABI
// declared in include/efe_engine.h, one file per concern (engine.h lists them).  The schedule follows
// SURVEY.md section 7 ("key scheduling insight"): depth and the MC loops are sequential only through
// the tiny transition net, so one call runs  (1) D small transition launches,  (2) ONE batched decoder
// pass over rows x D x 3S evaluations,  (3) ONE batched encoder pass over rows x D x S,  (4) a per-row
// term combine (engine_forward.hip run_core).
// This file: the registry of live contexts, and the entry points for a context's lifecycle, options,
// profiling and scratch management.
#include "engine.h"

namespace {

// frees everything a context owns (device of the context current); also the failure paths of efe_create_cfg
void release_ctx(efe_ctx* ctx) {
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    if (ctx->done_ev) (void)hipEventDestroy(ctx->done_ev);
    for (void* p : ctx->owned) (void)hipFree(p);
    for (void* p : ctx->wbufs) (void)hipFree(p);
    for (auto& b : ctx->arena.blocks) (void)hipFree(b.first);
    delete ctx;
}
// the registry's deleter: runs once efe_destroy has retired the context and its last admitted call has let go
void destroy_ctx(efe_ctx* ctx) {
    DeviceScope dev_scope_(ctx->device);
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    release_ctx(ctx);
}

}  // namespace

// the singletons of the host side: defined here and nowhere else
namespace efe {
namespace host {

// (While `st` is being captured into a hipGraph nothing executes: the event is not recorded -- an event recorded inside a capture may only
// be waited on inside it -- and the stream bookkeeping is left as it was; whoever replays the graph orders it against other streams.)
bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
// never destroyed: a context still live at exit is left to the process teardown, not released after the HIP runtime has shut down
CtxRegistry<efe_ctx>& registry() { static auto* r = new CtxRegistry<efe_ctx>(destroy_ctx); return *r; }
thread_local std::string tl_stale_msg;

}  // namespace host
}  // namespace efe

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" {

int efe_abi_version(void) { return 6; }

int efe_ctx_alive(const efe_ctx* ctx) { return registry().alive(ctx) ? 1 : 0; }

// efe_build_id(): the digest of the sources this library was compiled from -- a generated translation unit (build.py writes it at
// link time, so an edit of one kernel file recompiles that file only)

int efe_create(efe_ctx** out, int device) { return efe_create_cfg(out, device, 10, 4, 1, 64); }

int efe_create_cfg(efe_ctx** out, int device, int s_dim, int pi_dim, int channels, int resolution) {
    if (!out) return 1;
    *out = nullptr;
    // s_dim is 10 everywhere in the reference (train.py / test_demo.py); x rows are 16 floats = [pi | s | pad]
    if (s_dim != 10 || pi_dim < 2 || pi_dim > 6 || channels < 1 || channels > 3 || resolution < 32 || resolution > 128 || resolution % 4) return 7;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return 2;
    DeviceScope dev_scope_(device);                 // the caller's current device is restored on every exit
    if (hipSetDevice(device) != hipSuccess) return 3;
    if (init_small_kernels() || init_decoder_kernels() || init_fused_kernels() || init_train_kernels() || init_generic_kernels() || init_bf16x3_kernels()) return 5;       // per device: a second context on another GPU needs them too
    efe_ctx* ctx = new efe_ctx();
    ctx->device = device;
    ctx->pi_dim = pi_dim; ctx->chan = channels; ctx->res = resolution;
    ctx->generic = !(channels == 1 && resolution == 64);
    {   // the split simulation chain's cross-workgroup exchange (fused.hip: sc1 accesses, no fences) is validated on gfx950 only
        hipDeviceProp_t prop;
        ctx->arch_gfx950 = hipGetDeviceProperties(&prop, device) == hipSuccess && !strncmp(prop.gcnArchName, "gfx950", 6);
        if (!ctx->arch_gfx950) ctx->sim_split = 0;
    }
    ctx->last_s1 = resolution == 32;
    ctx->base = ctx->last_s1 ? resolution / 2 : resolution / 4;
    ctx->enc_hw[0] = resolution;
    for (int i = 1; i < 5; ++i) ctx->enc_hw[i] = (ctx->enc_hw[i - 1] - 3) / 2 + 1;      // Conv2d(k3, s2, p0), SURVEY appendix A.3
    if (ctx->enc_hw[4] < 1) { delete ctx; return 7; }
    if (ctx->generic) {
        const int64_t B = ctx->base, r = resolution;
        ctx->img_store = (size_t)r * r * GEN_IMG_LD;
        ctx->mac_dec = 10 * 256 + 2 * 256 * 256 + 256 * 64 * B * B + B * B * 9 * 64 * 64 * 2 + 4 * B * B * 9 * 64 * 32 + r * r * 9 * 32 * channels;
        // (the stride-1 third layer of the resolution-32 variant works on 2B x 2B inputs: the same 4 B^2 * 9 * 64 * 32 MACs)
        const int* hw = ctx->enc_hw;
        ctx->mac_enc = (int64_t)hw[1] * hw[1] * 9 * channels * 32 + (int64_t)hw[2] * hw[2] * 9 * 32 * 32 + (int64_t)hw[3] * hw[3] * 9 * 32 * 64
                     + (int64_t)hw[4] * hw[4] * 9 * 64 * 64 + (int64_t)hw[4] * hw[4] * 64 * 256 + 2 * 256 * 256 + 256 * 20;
    }
    ctx->mac_trans = (int64_t)(pi_dim + 10) * 512 + 2 * 512 * 512 + 512 * 20;
    ctx->mac_habit = 10 * 128 + 128 * 128 + 128 * pi_dim;
    // rows beyond the batch read their K operand values from this block (k_dense / k_conv_g): it must cover the longest contraction,
    // the encoder head's 64 * h4 * h4 inputs (3136 floats at resolution 128 -- an 8 KiB block was read past its end there)
    const size_t zeros_bytes = std::max<size_t>(8192, ((size_t)ctx->enc_hw[4] * ctx->enc_hw[4] * 64 + 64) * sizeof(float));
    // (every buffer enters ctx->owned right behind its hipMalloc and every failure path below releases through release_ctx(): nothing leaks)
    if (hipMalloc((void**)&ctx->zeros, zeros_bytes) != hipSuccess) { release_ctx(ctx); return 4; }
    ctx->owned.push_back(ctx->zeros);
    if (hipMemset(ctx->zeros, 0, zeros_bytes) != hipSuccess) { release_ctx(ctx); return 4; }
    if (hipEventCreateWithFlags(&ctx->done_ev, hipEventDisableTiming) != hipSuccess) { ctx->done_ev = nullptr; release_ctx(ctx); return 6; }
    {   // exchange buffer + counters of the split simulation chain (fused.hip k_sim_chain<8>)
        const size_t xb = (size_t)SIM_MAX_SPLIT_GROUPS * 2 * 16 * 512 * sizeof(float), sb = (size_t)SIM_MAX_SPLIT_GROUPS * 4 * sizeof(int);
        if (hipMalloc((void**)&ctx->sim_xch, xb) != hipSuccess) { release_ctx(ctx); return 4; }
        ctx->owned.push_back(ctx->sim_xch);
        if (hipMalloc((void**)&ctx->sim_sync, sb) != hipSuccess) { release_ctx(ctx); return 4; }
        ctx->owned.push_back(ctx->sim_sync);
        if (hipMemset(ctx->sim_sync, 0, sb) != hipSuccess) { release_ctx(ctx); return 4; }
    }
    {   // efe_eval_mi (eval_mi.hip): its workspace, and behind it the digamma table
        if (hipMalloc((void**)&ctx->mi_ws, (EVAL_MI_WS + EVAL_MI_PSI) * sizeof(double)) != hipSuccess) { release_ctx(ctx); return 4; }
        ctx->owned.push_back(ctx->mi_ws);
        std::vector<double> psi(EVAL_MI_PSI);
        eval_mi_psi_table(psi.data());
        if (hipMemcpy(ctx->mi_ws + EVAL_MI_WS, psi.data(), psi.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { release_ctx(ctx); return 4; }
    }
    registry().insert(ctx);
    *out = ctx;
    return 0;
}

void efe_destroy(efe_ctx* ctx) { registry().retire(ctx); }

int efe_get_config(efe_ctx* ctx, int* s_dim, int* pi_dim, int* channels, int* resolution) {
    Call call(ctx, Mode::host); if (!call) return 1;
    if (s_dim) *s_dim = S_DIM;
    if (pi_dim) *pi_dim = ctx->pi_dim;
    if (channels) *channels = ctx->chan;
    if (resolution) *resolution = ctx->res;
    return 0;
}

int efe_get_device(efe_ctx* ctx, int* device, char* pci_bus_id, int pci_bus_id_len) {
    Call call(ctx, Mode::host); if (!call) return 1;
    if (device) *device = ctx->device;
    if (pci_bus_id && pci_bus_id_len > 0) {
        pci_bus_id[0] = 0;
        if (hipDeviceGetPCIBusId(pci_bus_id, pci_bus_id_len, ctx->device) != hipSuccess) return ctx->fail("efe_get_device: hipDeviceGetPCIBusId failed");
    }
    return 0;
}

const char* efe_last_error(efe_ctx* ctx) {
    if (!ctx) return "null context";
    if (registry().alive(ctx)) return ctx->err.c_str();
    return tl_stale_msg.empty() ? "stale or invalid context handle" : tl_stale_msg.c_str();
}

int efe_set_option(efe_ctx* ctx, const char* name, int64_t value) {
    if (!name) return 1;
    Call call(ctx, Mode::host); if (!call) return 1;
    if (!strcmp(name, "dec_chunk")) { if (value < 1) return ctx->fail("dec_chunk < 1"); ctx->dec_chunk = value; return 0; }
    if (!strcmp(name, "reward_upstream_intent")) { ctx->reward_intent = value ? 1 : 0; return 0; }
    if (!strcmp(name, "ct_fuse12")) { ctx->ct_fuse12 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "enc_tiled")) { ctx->enc_tiled = value < 0 ? 0 : value > 2 ? 2 : value; return 0; }
    if (!strcmp(name, "fuse_final_g")) { ctx->fuse_final_g = value ? 1 : 0; return 0; }
    if (!strcmp(name, "dec_split")) { ctx->dec_split = value ? 1 : 0; return 0; }
    if (!strcmp(name, "dec_fuse_ab")) { ctx->dec_fuse_ab = value ? 1 : 0; return 0; }
    if (!strcmp(name, "dec_ab_grid")) { if (value < 0) return ctx->fail("dec_ab_grid < 0"); ctx->dec_ab_grid = value; return 0; }
    if (!strcmp(name, "dec_budget_g")) { if (value < (1 << 20)) return ctx->fail("dec_budget_g < 1 MiB"); ctx->dec_budget_g = value; return 0; }
    if (!strcmp(name, "dec_chunk_g")) { if (value < 1) return ctx->fail("dec_chunk_g < 1"); ctx->dec_chunk_g = value; return 0; }
    if (!strcmp(name, "poison")) { ctx->poison = value; return 0; }
    if (!strcmp(name, "trace")) { ctx->trace = value; return 0; }
    if (!strcmp(name, "check_rows")) { ctx->check_rows = value ? 1 : 0; return 0; }
    if (!strcmp(name, "sim_split")) {
        // the fence-free exchange of k_sim_chain<8> relies on gfx950's sc1 = agent-scope write-through / L2-bypassing accesses: refused elsewhere
        if (value && !ctx->arch_gfx950) return ctx->fail("sim_split: validated on gfx950 only (this device is another architecture)");
        ctx->sim_split = value ? 1 : 0; return 0;
    }
    if (!strcmp(name, "mfma_bf16x3") || !strcmp(name, "mfma_f16x2")) {       // opt-in experiments; the planes are packed now if the weights are already committed
        const int mode = !value ? 0 : name[5] == 'b' ? 1 : 2;
        if (mode && ctx->generic) return ctx->fail(std::string(name) + ": the experiment covers the Dynamic-dSprites geometry only");
        // (packed from ctx->raw only while raw IS the committed set -- efe_set_weight clears `committed`, the next commit packs the planes
        // with everything else; the option is on only after every plane exists: a failure part-way leaves the experiment off, not half-enabled)
        // A device-side step of ModelDown has made raw["down.*"] older than the master copy and has invalidated the planes (down_step clears
        // split_packed): the host tensors follow the master copy first, so the planes are those of the trained weights.
        if (mode && ctx->committed && ctx->split_packed != mode) {
            HIPCHK(hipSetDevice(ctx->device));
            HIPCHK(hipDeviceSynchronize());             // work that still reads the other mode's planes
            if (refresh_down_host(ctx)) return 1;
            if (pack_fc4_b3(ctx, mode)) { ctx->mfma_bf16x3 = 0; return 1; }
        }
        ctx->mfma_bf16x3 = mode;
        return 0;
    }
    if (!strcmp(name, "b3_convt3")) { ctx->b3_convt3 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "arena_align")) { if (value < 256 || (value & (value - 1))) return ctx->fail("arena_align must be a power of two >= 256"); ctx->arena_align = value; return 0; }
    if (!strcmp(name, "mid_unfused")) { ctx->mid_unfused = value; return 0; }
    if (!strcmp(name, "head_unfused")) { ctx->head_unfused = value; return 0; }
    if (!strcmp(name, "enc_chunk")) { if (value < 1) return ctx->fail("enc_chunk < 1"); ctx->enc_chunk = value; return 0; }
    return ctx->fail(std::string("unknown option ") + name);
}

int64_t efe_last_call_macs(efe_ctx* ctx) { Call call(ctx, Mode::host); return call ? ctx->last_macs : 0; }

int efe_prof_enable(efe_ctx* ctx, int on) {
    Call call(ctx, Mode::host); if (!call) return 1;
    ctx->prof = (on < 0) ? 0xFFFFFFFFu : (unsigned)on;       // < 0 = all classes, otherwise a bitmask (bit c = class c)
    ctx->ev_used = 0;
    ctx->ev_spans.clear();
    return 0;
}

int efe_prof_classes(void) { return PROF_NCLS; }

int efe_prof_read(efe_ctx* ctx, double* ms, int64_t* launches) {
    if (!ms || !launches) return 1;
    Call call(ctx, Mode::device); if (!call) return 1;
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < PROF_NCLS; ++i) { ms[i] = 0.0; launches[i] = 0; }
    for (auto& sp : ctx->ev_spans) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, sp.second.first, sp.second.second));
        ms[sp.first] += t; launches[sp.first] += 1;
    }
    ctx->ev_used = 0;
    ctx->ev_spans.clear();
    return 0;
}

// ---- scratch management --------------------------------------------------------------------------------
int efe_reserve(efe_ctx* ctx, int64_t bytes) {
    Call call(ctx, Mode::device); if (!call) return 1;
    if (bytes < 0) return ctx->fail("efe_reserve: bytes < 0");
    const size_t have = ctx->arena.capacity();
    if (ctx->arena.blocks.size() <= 1 && have >= (size_t)bytes) return 0;
    // one block that holds everything: a bump allocation never has to skip to the next block (no fragmentation, no growth)
    HIPCHK(hipDeviceSynchronize());
    for (auto& b : ctx->arena.blocks) (void)hipFree(b.first);
    ctx->arena.blocks.clear();
    ctx->arena.reset();
    const size_t sz = std::max((size_t)bytes, have);
    char* p = nullptr;
    if (hipMalloc((void**)&p, sz) != hipSuccess) return ctx->fail("efe_reserve: hipMalloc failed");
    ctx->arena.blocks.push_back({p, sz});
    return 0;
}

int64_t efe_rollout_scratch_bytes(efe_ctx* ctx, int M, int steps, int samples) {
    // the plans efe_rollout allocates from, nested as it calls them: its root with the root encode, then run_core.  Without a sum_terms
    // output (counted here) run_core takes 3 M floats that it does not take with one.
    Call call(ctx, Mode::host);
    if (!call || M < 1 || steps < 1 || samples < 1) return 0;
    return (int64_t)(plan_bytes(ctx, rollout_plan(ctx, M)) + encoder_bytes(ctx, M) + core_bytes(ctx, M, steps, samples, true) + SCRATCH_HEADROOM);
}

int efe_arena_stats(efe_ctx* ctx, int64_t* capacity_bytes, int64_t* high_water_bytes, int64_t* grow_count) {
    Call call(ctx, Mode::host); if (!call) return 1;
    if (capacity_bytes) *capacity_bytes = (int64_t)ctx->arena.capacity();
    if (high_water_bytes) *high_water_bytes = (int64_t)ctx->high_water;
    if (grow_count) *grow_count = ctx->arena_grows;
    return 0;
}

}  // extern "C"
