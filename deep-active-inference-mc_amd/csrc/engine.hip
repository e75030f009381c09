// Host side of the EFE rollout engine: context, weight packing, launch orchestration and the C ABI
// declared in include/efe_engine.h.  The schedule follows SURVEY.md section 7 ("key scheduling
// insight"): depth and the MC loops are sequential only through the tiny transition net, so one call
// runs  (1) D small transition launches,  (2) ONE batched decoder pass over rows x D x 3S evaluations,
// (3) ONE batched encoder pass over rows x D x S,  (4) a per-row term combine.
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

namespace {

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

}  // namespace

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
    float* enc_raw = nullptr;      // the whole qs_net unpacked, flat in parameters() order (kernels.h EQ_*): train_enc.hip reads it
    // ModelDown's master copy at 1 x 64 x 64 (owned: it outlives a re-commit, as TrainPart::master): [DOWN_P], qs_net then po_net, so
    // enc_raw = down_master and dec_raw = down_master + ENC_P.  An optimiser step (train_down.hip) writes it and rebuilds every packed form
    // of the table down_repack (device; one entry per packed buffer of pack_heads / pack_encoder / pack_decoder, built at commit).
    // down_dirty: the device copy is newer than raw["down.*"] (refresh_down_host).  dec_bf_stale: and newer than the host scalar dec_bf.
    float* down_master = nullptr;
    RepackDesc* down_repack = nullptr; int down_repack_n = 0, down_repack_blocks = 0;
    bool down_dirty = false, dec_bf_stale = false;
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

namespace {

// ---- weight packing ----------------------------------------------------------------------------------
// a host vector as a device buffer of the current commit (freed by the next one); nullptr with ctx->err set on failure
template <class T>
T* upload(efe_ctx* ctx, const std::vector<T>& v) {
    T* d = nullptr;
    if (hipMalloc((void**)&d, v.size() * sizeof(T)) != hipSuccess) { ctx->err = "weight upload: hipMalloc failed"; return nullptr; }
    ctx->wbufs.push_back(d);
    if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "weight upload: hipMemcpy failed"; return nullptr; }
    return d;
}

// a span of ModelDown's master copy (owned, allocated at the first commit of a 1 x 64 x 64 context): floats [off, off + v.size())
float* upload_master(efe_ctx* ctx, const std::vector<float>& v, size_t off) {
    if (!ctx->down_master) {
        if (hipMalloc((void**)&ctx->down_master, (size_t)DOWN_P * 4) != hipSuccess) { ctx->err = "master copy: hipMalloc failed"; return nullptr; }
        ctx->owned.push_back(ctx->down_master);
    }
    if (hipMemcpy(ctx->down_master + off, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "master copy: hipMemcpy failed"; return nullptr; }
    return ctx->down_master + off;
}

const HostTensor* need(efe_ctx* ctx, const std::string& key, std::initializer_list<int64_t> shape) {
    auto it = ctx->raw.find(key);
    if (it == ctx->raw.end()) { ctx->err = "missing weight " + key; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) { ctx->err = "bad shape for " + key; return nullptr; }
    return &it->second;
}
// key.weight and key.bias of one layer: both, or neither with need()'s message
struct WB {
    const HostTensor *w = nullptr, *b = nullptr;
    explicit operator bool() const { return w && b; }
    const float* W() const { return w->data.data(); }
    const float* B() const { return b->data.data(); }
};
WB weight_and_bias(efe_ctx* ctx, const std::string& key, std::initializer_list<int64_t> wshape, std::initializer_list<int64_t> bshape) {
    WB r;
    r.w = need(ctx, key + ".weight", wshape);
    if (r.w) r.b = need(ctx, key + ".bias", bshape);
    return r.b ? r : WB{};
}

// a layer from its already packed weights ([ntaps][mtiles][cin / 8][256], whatever the order inside) and its bias, padded to the tile count
int upload_layer(efe_ctx* ctx, Layer& L, int ntaps, int cout, int cin, const std::vector<float>& packed, const float* bias) {
    L.ntaps = ntaps; L.cout = cout; L.mtiles = (cout + 31) / 32; L.cin = (cin + 7) / 8 * 8;
    if (packed.size() != (size_t)ntaps * L.mtiles * (L.cin / 8) * 256) return ctx->fail("upload_layer: packed size does not match the layer");
    std::vector<float> b((size_t)L.mtiles * 32, 0.f);
    std::copy(bias, bias + cout, b.begin());
    L.Wp = upload(ctx, packed);
    L.bias = L.Wp ? upload(ctx, b) : nullptr;
    return L.bias ? 0 : 1;
}
// ... packed here into the MFMA fragment-major layout of v_mfma_f32_32x32x2_f32, [tap][mtile][kc][lane][4], from get(tap, co, ci)
template <class Get>
int upload_packed(efe_ctx* ctx, Layer& L, int ntaps, int cout, int cin, Get get, const float* bias) {
    const int mtiles = (cout + 31) / 32, KC = (cin + 7) / 8;
    std::vector<float> p((size_t)ntaps * mtiles * KC * 256);
    size_t idx = 0;
    for (int t = 0; t < ntaps; ++t)
        for (int mt = 0; mt < mtiles; ++mt)
            for (int kc = 0; kc < KC; ++kc)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const int co = mt * 32 + (lane & 31), ci = kc * 8 + 4 * (lane >> 5) + s;
                        p[idx++] = (co < cout && ci < cin) ? get(t, co, ci) : 0.f;
                    }
    return upload_layer(ctx, L, ntaps, cout, cin, p, bias);
}

// Minimal-filtering F(2, 2) weights of a stride-2 ConvTranspose2d(cin, cout, 3, s2, p1, op1), W [cin][cout][kh][kw] (kernels.h f22_*):
// U[4 wr + wc][co][ci] = sum_{kh, kw} f22_cw(wr, kh) f22_cw(wc, kw) W[ci][co][kh][kw], formed in fp64 and rounded once
std::vector<float> convt_s2_f22_weights(const float* W, int cin, int cout) {
    std::vector<float> U((size_t)16 * cout * cin);
    for (int wr = 0; wr < 4; ++wr)
        for (int wc = 0; wc < 4; ++wc)
            for (int co = 0; co < cout; ++co)
                for (int ci = 0; ci < cin; ++ci)
                    U[((size_t)(4 * wr + wc) * cout + co) * cin + ci] = f22_u_elem(W + ((size_t)ci * cout + co) * 9, wr, wc);
    return U;
}
// Winograd F(2x2, 3x3) weights of a stride-1 ConvTranspose2d(cin, cout, 3, s1, p1) (decoder.hip wino_l1): U[4 a + b][co][ci] = (G g G^T)[a][b]
// in fp64, rounded once; g[u][v] = W[ci][co][2 - u][2 - v] (the correlation form of the stride-1 transposed conv)
std::vector<float> convt_s1_wino_weights(const float* W, int cin, int cout) {
    // G = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}} (kernels.h wino_g; wino_u_elem forms one element, as the device repack does)
    std::vector<float> U((size_t)16 * cout * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b)
                    U[((size_t)(a * 4 + b) * cout + co) * cin + ci] = wino_u_elem(W + ((size_t)ci * cout + co) * 9, a, b);
    return U;
}
// 16 matrices U [cout][64] for v_mfma_f32_16x16x4_f32: [U][16-channel tile ct][chunk kc][lane][s] = U[16 ct + (lane & 15)][16 kc + 4 (lane >> 4) + s]
std::vector<float> pack_u16x16x4(const std::vector<float>& U, int cout) {
    const int T = cout / 16;
    std::vector<float> p(U.size());
    for (int m = 0; m < 16; ++m) for (int ct = 0; ct < T; ++ct) for (int kc = 0; kc < 4; ++kc) for (int lane = 0; lane < 64; ++lane)
        for (int s_ = 0; s_ < 4; ++s_)
            p[((((size_t)m * T + ct) * 4 + kc) * 64 + lane) * 4 + s_] = U[((size_t)m * cout + 16 * ct + (lane & 15)) * 64 + 16 * kc + 4 * (lane >> 4) + s_];
    return p;
}
// torch's Flatten / Unflatten index a [channels][positions] block channel-major, c * positions + p; the kernels keep it NHWC, p * channels + c:
// perm[NHWC index] = channel-major index
std::vector<int> nhwc_perm(int channels, int positions) {
    std::vector<int> perm((size_t)positions * channels);
    for (int p = 0; p < positions; ++p) for (int c = 0; c < channels; ++c) perm[(size_t)p * channels + c] = c * positions + p;
    return perm;
}

// (LayerSpec: one layer of a network as the weight tables below list it: a Linear(in, out), or a 3 x 3 convolution (out = cout, in = cin))
constexpr int TOP_NL = 3, MID_NL = 4;
const char* const TOP_KEYS[TOP_NL] = {"top.qpi_net.0", "top.qpi_net.2", "top.qpi_net.4"};
// habit net (torchmodel.py:19-25)
LayerSpec top_layer(int i, int A) { const int out[TOP_NL] = {128, 128, A}, in[TOP_NL] = {10, 128, 128}; return {TOP_KEYS[i], out[i], in[i]}; }
// transition net (torchmodel.py:41-52); input = cat[pi, s0] (torchmodel.py:59)
LayerSpec mid_layer(int i, int A) {
    const LayerSpec t[MID_NL] = {{"mid.ps_net.0", 512, A + 10}, {"mid.ps_net.3", 512, 512}, {"mid.ps_net.6", 512, 512}, {"mid.ps_net.9", 20, 512}};
    return t[i];
}
// decoder head; encoder head behind its first layer (whose width follows the geometry: pack_encoder)
const LayerSpec DEC_HEAD[3] = {{"down.po_net.0", 256, 10}, {"down.po_net.3", 256, 256}, {"down.po_net.6", 256, 256}};
const LayerSpec ENC_HEAD[3] = {{"down.qs_net.12", 256, 256}, {"down.qs_net.15", 256, 256}, {"down.qs_net.18", 20, 256}};
// encoder Conv2d stack (torchmodel.py:84-104; layer 0 reads the image's channels) and decoder ConvTranspose2d stack
LayerSpec enc_conv_layer(int i, int C) { const LayerSpec t[4] = {{"down.qs_net.0", 32, C}, {"down.qs_net.2", 32, 32}, {"down.qs_net.4", 64, 32}, {"down.qs_net.6", 64, 64}}; return t[i]; }
const LayerSpec DEC_CT[3] = {{"down.po_net.13", 64, 64}, {"down.po_net.15", 64, 64}, {"down.po_net.17", 32, 64}};

int pack_linear(efe_ctx* ctx, Layer& L, const LayerSpec& s, const int* row_perm = nullptr, const int* col_perm = nullptr) {
    const WB t = weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
    if (!t) return 1;
    const float* W = t.W();
    const int in = s.in;
    std::vector<float> b((size_t)s.out);
    for (int co = 0; co < s.out; ++co) b[co] = t.B()[row_perm ? row_perm[co] : co];
    return upload_packed(ctx, L, 1, s.out, in,
        [&](int, int co, int ci) { return W[(size_t)(row_perm ? row_perm[co] : co) * in + (col_perm ? col_perm[ci] : ci)]; }, b.data());
}

// packed for v_mfma_f32_16x16x4_f32 (fused.hip): [16-feature tile][16-channel chunk][lane = (m, q)][s] = W[16 mt + m][16 kc + 4 q + s]
int pack_linear16(efe_ctx* ctx, MlpW& net, int layer, const LayerSpec& s, const int* col_perm = nullptr) {
    const WB t = weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
    if (!t) return 1;
    const int out = s.out, in = s.in, mtiles = (out + 15) / 16, KC = (in + 15) / 16;
    std::vector<float> p((size_t)mtiles * KC * 256, 0.f), bb((size_t)mtiles * 16, 0.f);
    for (int mt = 0; mt < mtiles; ++mt)
        for (int kc = 0; kc < KC; ++kc)
            for (int lane = 0; lane < 64; ++lane)
                for (int s_ = 0; s_ < 4; ++s_) {
                    const int co = 16 * mt + (lane & 15), ci = 16 * kc + 4 * (lane >> 4) + s_;
                    if (co < out && ci < in) p[(((size_t)mt * KC + kc) * 64 + lane) * 4 + s_] = t.W()[(size_t)co * in + (col_perm ? col_perm[ci] : ci)];
                }
    std::copy(t.B(), t.B() + out, bb.begin());
    const float* dW = upload(ctx, p);
    const float* dB = dW ? upload(ctx, bb) : nullptr;
    if (!dB) return 1;
    net.w[layer] = reinterpret_cast<const float4*>(dW); net.b[layer] = dB;
    return 0;
}
// a 3 x 3 Conv2d (W [cout][cin][3][3]) or ConvTranspose2d (W [cin][cout][3][3]) as nine taps of the 32x32x2 form
int pack_conv(efe_ctx* ctx, Layer& L, const LayerSpec& s, bool transposed) {
    const WB t = transposed ? weight_and_bias(ctx, s.key, {s.in, s.out, 3, 3}, {s.out}) : weight_and_bias(ctx, s.key, {s.out, s.in, 3, 3}, {s.out});
    if (!t) return 1;
    const float* W = t.W();
    const int cin = s.in, cout = s.out;
    if (transposed) return upload_packed(ctx, L, 9, cout, cin, [&](int tap, int co, int ci) { return W[((size_t)ci * cout + co) * 9 + tap]; }, t.B());
    return upload_packed(ctx, L, 9, cout, cin, [&](int tap, int co, int ci) { return W[((size_t)co * cin + ci) * 9 + tap]; }, t.B());
}

// ---- training tables (train.hip) ---------------------------------------------------------------------
int part_param_count(int nl, LayerSpec (*layer)(int, int), int A) { int n = 0; for (int i = 0; i < nl; ++i) { const LayerSpec s = layer(i, A); n += s.out * s.in + s.out; } return n; }

// a trainable part's master copy and layer table, after its packed forms exist (pack_net): the gradient kernel reads the master copy
// (k_mid_grad: and the 16x16x4 copy), k_adam writes it and both packed copies.  drop_tag0 != 0: every hidden layer is followed by
// MC-dropout under tag drop_tag0 + layer.
int build_train(efe_ctx* ctx, TrainPart& tp, const char* prefix, int nl, LayerSpec (*layer)(int, int), const Layer* L32, const MlpW& L16, uint32_t drop_tag0) {
    const int A = ctx->pi_dim;
    TrainNet nt{};
    nt.nl = nl;
    std::vector<float> flat;
    for (int i = 0; i < nl; ++i) {
        const LayerSpec s = layer(i, A);
        const WB t = weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
        if (!t) return 1;
        TrainLayer& L = nt.L[i];
        L.in = s.in; L.out = s.out; L.relu = i < nl - 1; L.drop_tag = (drop_tag0 && i < nl - 1) ? (int)drop_tag0 + i : 0;
        L.w_off = (int)flat.size(); flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
        L.b_off = (int)flat.size(); flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        L.kc32 = L32[i].cin / 8; L.kc16 = (s.in + 15) / 16;
        L.Wp32 = L32[i].Wp; L.b32 = L32[i].bias;
        L.Wp16 = const_cast<float*>(reinterpret_cast<const float*>(L16.w[i])); L.b16 = const_cast<float*>(L16.b[i]);
    }
    nt.P = (int)flat.size();
    if (!tp.master) {
        HIPCHK(hipMalloc((void**)&tp.master, (size_t)nt.P * 4)); ctx->owned.push_back(tp.master);
        HIPCHK(hipMalloc((void**)&tp.net_dev, sizeof(TrainNet))); ctx->owned.push_back(tp.net_dev);
    }
    nt.master = tp.master;
    HIPCHK(hipMemcpy(tp.master, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tp.net_dev, &nt, sizeof(TrainNet), hipMemcpyHostToDevice));
    tp.net = nt; tp.nl = nl; tp.layer = layer; tp.prefix = prefix;
    tp.dirty = false;
    return 0;
}
int build_top_train(efe_ctx* ctx) {
    if (ctx->pi_dim > TRAIN_MAX_A) return ctx->fail("habit net outside the training kernels' limits");
    return build_train(ctx, ctx->top_train, "top.", TOP_NL, top_layer, ctx->top, ctx->top16, 0u);
}
// k_mid_grad's LDS map: one 16-channel input chunk, hidden layers of TRAIN_MID_WIDTH (whole 16-feature tiles), mean | logvar out
int build_mid_train(efe_ctx* ctx) {
    static_assert(MID_NL == TRAIN_MAX_LAYERS, "k_mid_grad keeps one LDS buffer per hidden layer of the table");
    for (int i = 0; i < MID_NL; ++i) {
        const LayerSpec s = mid_layer(i, ctx->pi_dim);
        if ((i == 0 ? s.in > TRAIN_MID_IN : s.in != TRAIN_MID_WIDTH) || (i < MID_NL - 1 ? s.out != TRAIN_MID_WIDTH : s.out != 2 * S_DIM))
            return ctx->fail("transition net outside the training kernel's limits");
    }
    return build_train(ctx, ctx->mid_train, "mid.", MID_NL, mid_layer, ctx->mid, ctx->mid16, TAG_MID);
}

// an optimiser step has made the device master copy newer than the host tensors: bring them up to date (synchronises), so that neither
// a re-commit nor a partial efe_set_weight of the part reverts what was learnt
int refresh_train_host(efe_ctx* ctx, TrainPart& tp) {
    if (!tp.dirty) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    const TrainNet& nt = tp.net;
    std::vector<float> flat((size_t)nt.P);
    HIPCHK(hipMemcpy(flat.data(), tp.master, flat.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < nt.nl; ++i) {
        const TrainLayer& L = nt.L[i];
        const std::string key = tp.layer(i, ctx->pi_dim).key;
        auto& w = ctx->raw[key + ".weight"].data;
        auto& b = ctx->raw[key + ".bias"].data;
        w.assign(flat.begin() + L.w_off, flat.begin() + L.w_off + (size_t)L.out * L.in);
        b.assign(flat.begin() + L.b_off, flat.begin() + L.b_off + L.out);
    }
    tp.dirty = false;
    return 0;
}

// ... and the same for ModelDown's master copy (efe_train_down / efe_down_adam_step): all 32 tensors of raw["down.*"], in parameters() order
const char* const DOWN_KEYS[16] = {"down.qs_net.0", "down.qs_net.2", "down.qs_net.4", "down.qs_net.6", "down.qs_net.9", "down.qs_net.12", "down.qs_net.15",
                                   "down.qs_net.18", "down.po_net.0", "down.po_net.3", "down.po_net.6", "down.po_net.9", "down.po_net.13", "down.po_net.15",
                                   "down.po_net.17", "down.po_net.19"};
int refresh_down_host(efe_ctx* ctx) {
    if (!ctx->down_dirty) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<float> flat((size_t)DOWN_P);
    HIPCHK(hipMemcpy(flat.data(), ctx->down_master, flat.size() * 4, hipMemcpyDeviceToHost));
    size_t off = 0;
    for (const char* key : DOWN_KEYS)
        for (const char* sfx : {".weight", ".bias"}) {
            auto it = ctx->raw.find(std::string(key) + sfx);
            if (it == ctx->raw.end() || off + it->second.data.size() > flat.size()) return ctx->fail(std::string("master copy: no host tensor to refresh for ") + key + sfx);
            std::vector<float>& d = it->second.data;
            d.assign(flat.begin() + off, flat.begin() + off + d.size());
            off += d.size();
        }
    if (off != flat.size()) return ctx->fail("master copy: the host tensors do not add up to the parameter count");
    ctx->dec_bf = flat.back(); ctx->dec_bf_stale = false;
    ctx->down_dirty = false;
    return 0;
}

// the table k_repack_down works from (train_down.hip): one entry per packed buffer and bias table that pack_heads, pack_encoder and
// pack_decoder fill on the 1 x 64 x 64 path, with the buffers of THIS commit; its kinds name the packers they invert
int build_down_repack(efe_ctx* ctx) {
    std::vector<RepackDesc> t;
    int blocks = 0;
    auto add = [&](float* dst, int src, int kind, int n, int out, int in, int KC, int mtiles, int row_ch = 0, int row_pos = 0, int col_ch = 0, int col_pos = 0) {
        RepackDesc d{};
        d.dst = dst; d.src = src; d.kind = kind; d.n = n; d.block0 = blocks; d.out = out; d.in = in; d.KC = KC; d.mtiles = mtiles;
        d.row_ch = row_ch; d.row_pos = row_pos; d.col_ch = col_ch; d.col_pos = col_pos;
        d.vec = (kind == RP_DENSE32 || kind == RP_DENSE16) && !col_ch && src % 4 == 0 && in % (kind == RP_DENSE32 ? 8 : 16) == 0;
        d.swizzle = kind == RP_DENSE32 && d.vec && KC % 4 == 0;
        blocks += (n + 255) / 256;
        t.push_back(d);
    };
    auto bias = [&](float* dst, int src, int out, int n, int row_ch = 0, int row_pos = 0) { add(dst, src, RP_BIAS, n, out, 0, 0, 0, row_ch, row_pos); };
    auto dense32 = [&](const Layer& L, int w, int b, int out, int in, int row_ch = 0, int row_pos = 0, int col_ch = 0, int col_pos = 0) {
        add(L.Wp, w, RP_DENSE32, L.mtiles * (L.cin / 8) * 64, out, in, L.cin / 8, L.mtiles, row_ch, row_pos, col_ch, col_pos);
        bias(L.bias, b, out, L.mtiles * 32, row_ch, row_pos);
    };
    auto dense16 = [&](const MlpW& net, int layer, int w, int b, int out, int in, int col_ch = 0, int col_pos = 0) {
        const int mtiles = (out + 15) / 16, KC = (in + 15) / 16;
        add(const_cast<float*>(reinterpret_cast<const float*>(net.w[layer])), w, RP_DENSE16, mtiles * KC * 64, out, in, KC, mtiles, 0, 0, col_ch, col_pos);
        bias(const_cast<float*>(net.b[layer]), b, out, mtiles * 16);
    };
    const int D = ENC_P, T = ENC_P + DEC_HEAD_P;      // po_net and its ConvT tail inside the master copy
    // pack_heads
    const int dh[3][4] = {{DH_W0, DH_B0, 256, 10}, {DH_W1, DH_B1, 256, 256}, {DH_W2, DH_B2, 256, 256}};
    const int eh[3][4] = {{EQ_W12, EQ_B12, 256, 256}, {EQ_W15, EQ_B15, 256, 256}, {EQ_W18, EQ_B18, 20, 256}};
    for (int i = 0; i < 3; ++i) {
        dense32(ctx->dec_fc[i], D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]); dense16(ctx->dec16, i, D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]);
        dense32(ctx->enc_fc[i + 1], eh[i][0], eh[i][1], eh[i][2], eh[i][3]); dense16(ctx->enc16, i + 1, eh[i][0], eh[i][1], eh[i][2], eh[i][3]);
    }
    // pack_encoder: conv1 on the VALU, conv2 / conv3 as nine taps of the 32x32x2 form, conv4 in the 16x16x4 form, the head's first layer (columns NHWC)
    add(ctx->enc_w1, EQ_W1, RP_TAP32, 288, 32, 1, 0, 0); bias(ctx->enc_b1, EQ_B1, 32, 32);
    add(ctx->enc_conv[0].Wp, EQ_W2, RP_CONV32, 9 * 1 * 4 * 64, 32, 32, 4, 1); bias(ctx->enc_conv[0].bias, EQ_B2, 32, 32);
    add(ctx->enc_conv[1].Wp, EQ_W3, RP_CONV32, 9 * 2 * 4 * 64, 64, 32, 4, 2); bias(ctx->enc_conv[1].bias, EQ_B3, 64, 64);
    add(ctx->enc_conv[2].Wp, EQ_W4, RP_CONV16, 9 * 4 * 4 * 64, 64, 64, 4, 4); bias(ctx->enc_conv[2].bias, EQ_B4, 64, 64);
    dense32(ctx->enc_fc[0], EQ_W9, EQ_B9, 256, 576, 0, 0, 64, 9); dense16(ctx->enc16, 0, EQ_W9, EQ_B9, 256, 576, 64, 9);
    // pack_decoder: Linear(256, 16384) with its rows NHWC, the Winograd and F(2, 2) matrices, the final convolution (its bias: ctx->dec_bf)
    dense32(ctx->dec_fc[3], D + DH_W3, D + DH_B3, 16384, 256, 64, 256);
    add(ctx->dec_ct[0].Wp, T + DT_W1, RP_WINO, 16 * 2 * 8 * 64, 64, 64, 8, 2); bias(ctx->dec_ct[0].bias, T + DT_B1, 64, 64);
    add(ctx->dec_ct[1].Wp, T + DT_W2, RP_F22, 16 * 4 * 4 * 64, 64, 64, 4, 4); bias(ctx->dec_ct[1].bias, T + DT_B2, 64, 64);
    add(ctx->dec_ct[2].Wp, T + DT_W3, RP_F22, 16 * 2 * 4 * 64, 32, 64, 4, 2); bias(ctx->dec_ct[2].bias, T + DT_B3, 32, 32);
    add(ctx->dec_wf, T + DT_W4, RP_TAP32, 288, 32, 1, 0, 0);
    constexpr size_t CAP = 64;
    if (t.size() > CAP) return ctx->fail("repack table: more entries than its buffer holds");
    for (const RepackDesc& d : t) if (!d.dst) return ctx->fail("repack table: a packed buffer is missing");
    if (!ctx->down_repack) {
        HIPCHK(hipMalloc((void**)&ctx->down_repack, CAP * sizeof(RepackDesc))); ctx->owned.push_back(ctx->down_repack);
    }
    HIPCHK(hipMemcpy(ctx->down_repack, t.data(), t.size() * sizeof(RepackDesc), hipMemcpyHostToDevice));
    ctx->down_repack_n = (int)t.size(); ctx->down_repack_blocks = blocks;
    return 0;
}

// ---- launch helpers ----------------------------------------------------------------------------------
struct NoiseCfg {
    uint32_t k0 = 0, k1 = 0;
    GroupMap gm{1, 1, {0, 0, 0}, 0, 0};
    int rows_per_group = 1;
    uint32_t row_offset = 0;
    const uint8_t* mask = nullptr;      // liveness of the logical rows (efe_rows.mask), entry = row / mask_div
    int mask_div = 1;
};
inline RowMask live_of(const NoiseCfg& nc, int m0) { return RowMask{nc.mask, nc.mask_div, m0, nc.rows_per_group, nc.mask ? nc.gm.ids : nullptr}; }
// the noise addressing of one network pass: key words, rows per group and this rank's row offset, the group -> (pass, sample, stage) map,
// and optionally the row identities / liveness mask of an efe_rows call (one entry = div rows)
NoiseCfg make_noise(uint32_t k0, uint32_t k1, int rows_per_group, uint32_t row_offset, GroupMap gm, const int32_t* ids = nullptr, int div = 1,
                    const uint8_t* mask = nullptr) {
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
// the six noise-addressing fields that GemmArgs, HeadArgs and TransFusedArgs share by name
template <class Args>
void set_keys(Args& a, const NoiseCfg& nc, int m0) {
    a.k0 = nc.k0; a.k1 = nc.k1; a.gm = nc.gm; a.rows_per_group = nc.rows_per_group; a.row_offset = nc.row_offset; a.m0 = m0;
}

// The profiling span of one launch: the launches of its scope count under class `cls` (efe_prof_read), between two events on the stream when
// that class is being timed.  The end of the scope closes the span and puts the class back; cancel() = nothing was launched, record no span.
struct ProfSpan {
    efe_ctx* const ctx; const hipStream_t st; const int prev; hipEvent_t e0;
    ProfSpan(efe_ctx* c, int cls, hipStream_t s) : ctx(c), st(s), prev(c->cls) { c->cls = cls; e0 = c->prof_begin(s); }
    void cancel() { e0 = nullptr; }
    ~ProfSpan() { ctx->prof_end(e0, st); ctx->cls = prev; }
};

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
struct DecPlan { int C; bool split; size_t hA, hB, x4, y2, queues; };       // queues: one image-ticket counter (int) per k_dec_a launch
DecPlan dec_plan(const efe_ctx* ctx, int64_t N) {
    const int64_t C = std::min<int64_t>(ctx->dec_chunk, N);
    return {(int)C, dec_split(ctx, N), (size_t)N * 256, (size_t)N * 256, (size_t)C * 16384, (size_t)C * 65536, (size_t)((N + C - 1) / C)};
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

// the root of efe_rollout: the encoded observation, the first transition input, and (generic geometry) the observation as NHWC4
struct RolloutPlan { size_t enc0, x, o8; };
RolloutPlan rollout_plan(const efe_ctx* ctx, int64_t M) { return {(size_t)M * 32, (size_t)M * 16, ctx->generic ? (size_t)M * ctx->img_store : 0}; }
size_t plan_bytes(const efe_ctx* c, const RolloutPlan& p) { return arena_bytes(c, {p.enc0, p.x, p.o8}); }

// efe_dec_tail_grad (train_dec.hip): the stored activations and the gradients of one row group (C rows; y_l / po exist only when the caller
// gives no output for them), nlogpo1 never (required output), and the partial-gradient slabs (none at G = 1: the gradient itself)
struct DecTailPlan { int C, G; size_t y1, y2, y3, po, g4, g3, g2, g1, slabs; };
DecTailPlan dec_tail_plan(int64_t M, bool own_y1, bool own_y2, bool own_y3, bool own_po) {
    const size_t C = (size_t)std::min<int64_t>(DEC_TAIL_ROWS, M);
    const int G = dec_tail_slabs((int)std::min<int64_t>(M, DEC_TAIL_SLABS));
    return {(int)C, G, own_y1 ? C * DEC_TAIL_Y1 : 0, own_y2 ? C * DEC_TAIL_Y2 : 0, own_y3 ? C * DEC_TAIL_Y3 : 0, own_po ? C * 4096 : 0,
            C * 4096, C * DEC_TAIL_Y3, C * DEC_TAIL_Y2, C * DEC_TAIL_Y1, G > 1 ? (size_t)G * DEC_TAIL_P : 0};
}
size_t plan_bytes(const efe_ctx* c, const DecTailPlan& p) { return arena_bytes(c, {p.y1, p.y2, p.y3, p.po, p.g4, p.g3, p.g2, p.g1, p.slabs}); }

// efe_dec_grad (train_dec_head.hip) on top of the tail's plan: the head's stored activations of one row group (those the caller gives no
// output for), d_h4 (gated in place to layer 3's gradient), the 64 segment partials of d_h3, and the slabs of layers 0..2 (none at G = 1)
struct DecHeadPlan { int C, G; size_t h1, h2, h3, h4, dh4, part, slabs; };
DecHeadPlan dec_head_plan(int64_t M, bool own_h1, bool own_h2, bool own_h3, bool own_h4) {
    const size_t C = (size_t)std::min<int64_t>(DEC_TAIL_ROWS, M);
    const int G = dec_head_slabs((int)std::min<int64_t>(M, 16 * DEC_HEAD_SLABS));
    return {(int)C, G, own_h1 ? C * 256 : 0, own_h2 ? C * 256 : 0, own_h3 ? C * 256 : 0, own_h4 ? C * DEC_TAIL_Y1 : 0, C * DEC_TAIL_Y1,
            (size_t)DEC_HEAD_SEGS * C * 256, G > 1 ? (size_t)G * DEC_HEAD_SMALL_P : 0};
}

// the sums, nested as the calls are: run_decoder / run_encoder dispatch on the geometry, run_core runs D transitions and one pass of each
size_t decoder_bytes(const efe_ctx* ctx, int64_t N) { return ctx->generic ? plan_bytes(ctx, dec_g_plan(ctx, N)) : plan_bytes(ctx, dec_plan(ctx, N)); }
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

// generic geometry (generic.hip): dense head -> Linear(256, 64*B*B) -> ConvT(64,64,s1) -> ConvT(64,64,s2) -> ConvT(64,32,s2) -> final conv
int run_decoder_g(efe_ctx* ctx, const float* dec_in, int N, const NoiseCfg& nc, int reward0, int store0, float* val, float* po_store,
                  hipStream_t st) {
    const int B = ctx->base, H2 = 2 * B, H3 = ctx->last_s1 ? 2 * B : 4 * B;
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

// ModelDown.po_net over N rows ([group][row] batch): the three small dense layers run once over all rows, then per
// chunk: dense 256->16384 (+dropout) -> k_dec_a (two transposed convs through LDS) -> k_dec_b (third transposed conv,
// final conv, sigmoid and the per-image reduction, all on chip).
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

// (While `st` is being captured into a hipGraph nothing executes: the event is not recorded -- an event recorded inside a capture may only
// be waited on inside it -- and the stream bookkeeping is left as it was; whoever replays the graph orders it against other streams.)
inline bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive;
}
// puts the caller's device back on exit if it is not `dev` (< 0: none): a call on a context of GPU 1 must not leave the thread on GPU 1
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int dev) { int cur = -1; if (dev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != dev) prev = cur; }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
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
// never destroyed: a context still live at exit is left to the process teardown, not released after the HIP runtime has shut down
CtxRegistry<efe_ctx>& registry() { static auto* r = new CtxRegistry<efe_ctx>(destroy_ctx); return *r; }

// The scope of one C ABI call: it admits the handle (ctx->mu held to its end) and puts the caller's device back on every exit.  Modes: host,
// nothing more; device, the context's device made current; scratch, that and a call on the scratch arena on stream `st`: work of the previous
// call still in flight on ANOTHER stream finishes first (same stream: stream order guarantees it), and every exit after that -- success or
// failure, kernels maybe queued -- records done_ev behind `st`'s work, so that the next call, on any stream, can order its arena reuse behind it.
// false: a refused handle (return code 1, efe_last_error explains) or a failed start (its message in ctx->err).
enum class Mode { host, device, scratch };
// what efe_last_error says of a handle that is not live, on this thread: the plain message, or (Call::refused) the one that names the entry
// point which was just handed it; every new call scope puts the plain one back
thread_local std::string tl_stale_msg;
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
        if (mode != Mode::scratch) return 0;
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

int mcts_tree(efe_ctx* ctx, const efe_mcts_tree* t, MctsTree& o) {
    if (!t || !t->W || !t->N || !t->Qpi || !t->child || !t->S || t->E < 1 || t->cap < 1 || t->A < 1 || t->A > 8 || t->s_dim < 1)
        return ctx->fail("efe_mcts: bad tree");
    o = MctsTree{t->W, t->N, t->Qpi, t->child, t->S, t->E, t->cap, t->A, t->s_dim};
    return 0;
}

// ---- training-side free energy (loss.hip) -------------------------------------------------------------
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
}  // namespace

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

int efe_set_weight(efe_ctx* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim) {
    if (!key || !data_host || !shape || ndim < 1 || ndim > 4) return 1;
    Call call(ctx, Mode::host); if (!call) return 1;
    for (TrainPart* tp : {&ctx->top_train, &ctx->mid_train})       // the other tensors of a trained part keep what was learnt
        if (tp->dirty && !strncmp(key, tp->prefix, strlen(tp->prefix)) && refresh_train_host(ctx, *tp)) return 1;
    if (ctx->down_dirty && !strncmp(key, "down.", 5) && refresh_down_host(ctx)) return 1;
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data_host, data_host + n);
    ctx->raw[key] = std::move(t);
    ctx->committed = false;
    return 0;
}

static int pack_fc4_b3(efe_ctx* ctx, int mode);

int efe_set_option(efe_ctx* ctx, const char* name, int64_t value) {
    if (!name) return 1;
    Call call(ctx, Mode::host); if (!call) return 1;
    if (!strcmp(name, "dec_chunk")) { if (value < 1) return ctx->fail("dec_chunk < 1"); ctx->dec_chunk = value; return 0; }
    if (!strcmp(name, "reward_upstream_intent")) { ctx->reward_intent = value ? 1 : 0; return 0; }
    if (!strcmp(name, "ct_fuse12")) { ctx->ct_fuse12 = value ? 1 : 0; return 0; }
    if (!strcmp(name, "enc_tiled")) { ctx->enc_tiled = value < 0 ? 0 : value > 2 ? 2 : value; return 0; }
    if (!strcmp(name, "fuse_final_g")) { ctx->fuse_final_g = value ? 1 : 0; return 0; }
    if (!strcmp(name, "dec_split")) { ctx->dec_split = value ? 1 : 0; return 0; }
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

// options mfma_bf16x3 (mode 1) / mfma_f16x2 (mode 2): po_net.9 (rows in NHWC order), po_net.13 / .15 / .17 as 16-bit planes for the kernels of
// bf16x3.hip.  Planes of the other mode are released first; a failure leaves no planes at all.
static void drop_split_planes(efe_ctx* ctx) {
    void* old[4] = {ctx->fc4_b3, ctx->ct_b3[0], ctx->ct_b3[1], ctx->ct3_b3};
    for (void* q : old) {
        if (!q) continue;
        ctx->wbufs.erase(std::remove(ctx->wbufs.begin(), ctx->wbufs.end(), q), ctx->wbufs.end());
        (void)hipFree(q);
    }
    ctx->fc4_b3 = nullptr; ctx->ct_b3[0] = ctx->ct_b3[1] = nullptr; ctx->ct3_b3 = nullptr; ctx->split_packed = 0;
}
static int pack_fc4_b3(efe_ctx* ctx, int mode) {
    drop_split_planes(ctx);
    const int npl = mode == 2 ? 2 : 3;
    auto fail = [&](const char* what) { drop_split_planes(ctx); return ctx->fail(std::string("split-operand planes: ") + what); };
    const HostTensor* w = need(ctx, "down.po_net.9.weight", {16384, 256});
    if (!w) { drop_split_planes(ctx); return 1; }
    const std::vector<int> rowp = nhwc_perm(64, 256);
    std::vector<uint16_t> planes((size_t)16384 * 256 * npl);
    ctx->s_fc4 = pack_dense_split(mode, w->data.data(), rowp.data(), 16384, 256, planes.data());
    if (!(ctx->fc4_b3 = upload(ctx, planes))) return fail("po_net.9");
    for (int i = 0; i < 3; ++i) {
        const LayerSpec& s = DEC_CT[i];
        const HostTensor* cw = need(ctx, std::string(s.key) + ".weight", {s.in, s.out, 3, 3});
        if (!cw) { drop_split_planes(ctx); return 1; }
        if (i < 2) {
            std::vector<uint16_t> cp((size_t)9 * 64 * 64 * npl);
            ctx->s_ct[i] = pack_conv_split(mode, cw->data.data(), 64, 64, cp.data());
            if (!(ctx->ct_b3[i] = upload(ctx, cp))) return fail(s.key);
        } else {
            std::vector<uint16_t> cp((size_t)4 * 9 * npl * 64 * 8);
            ctx->s_ct3 = pack_convt3_split(mode, cw->data.data(), cp.data());
            if (!(ctx->ct3_b3 = upload(ctx, cp))) return fail(s.key);
        }
    }
    ctx->split_packed = mode;
    return 0;
}

// a dense net in both packed forms: 32x32x2 tiles for k_dense (the layer-by-layer path) and 16x16x4 tiles for the fused kernels
static int pack_net(efe_ctx* ctx, int nl, LayerSpec (*layer)(int, int), Layer* L32, MlpW& L16) {
    for (int i = 0; i < nl; ++i) {
        const LayerSpec s = layer(i, ctx->pi_dim);
        if (pack_linear(ctx, L32[i], s) || pack_linear16(ctx, L16, i, s)) return 1;
    }
    return 0;
}
static int pack_top(efe_ctx* ctx) { return pack_net(ctx, TOP_NL, top_layer, ctx->top, ctx->top16) || build_top_train(ctx); }
static int pack_mid(efe_ctx* ctx) { return pack_net(ctx, MID_NL, mid_layer, ctx->mid, ctx->mid16) || build_mid_train(ctx); }
// the geometry-independent dense layers of the decoder / encoder heads (the encoder's first layer: pack_encoder)
static int pack_heads(efe_ctx* ctx) {
    for (int i = 0; i < 3; ++i) {
        if (pack_linear(ctx, ctx->dec_fc[i], DEC_HEAD[i]) || pack_linear16(ctx, ctx->dec16, i, DEC_HEAD[i])) return 1;
        if (pack_linear(ctx, ctx->enc_fc[i + 1], ENC_HEAD[i]) || pack_linear16(ctx, ctx->enc16, i + 1, ENC_HEAD[i])) return 1;
    }
    return 0;
}
// encoder (torchmodel.py:84-104): the convolution stack, then the head's first layer
static int pack_encoder(efe_ctx* ctx) {
    const int C = ctx->chan, F = ctx->enc_hw[4] * ctx->enc_hw[4];
    ctx->enc_raw = nullptr;
    if (C == 1 && ctx->res == 64) {     // the raw copy the training forward and backward read (train_enc.hip), beside the packed forward forms
        std::vector<float> flat;
        for (int i = 0; i < 8; ++i) {
            const LayerSpec s = i < 4 ? enc_conv_layer(i, C) : i == 4 ? LayerSpec{"down.qs_net.9", 256, F * 64} : ENC_HEAD[i - 5];
            const WB t = i < 4 ? weight_and_bias(ctx, s.key, {s.out, s.in, 3, 3}, {s.out}) : weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (flat.size() != (size_t)ENC_P) return ctx->fail("encoder: unexpected parameter count");
        if (!(ctx->enc_raw = upload_master(ctx, flat, 0))) return 1;
    }
    if (ctx->generic) {     // build-defined geometry: four k_conv_g layers ...
        for (int i = 0; i < 4; ++i) if (pack_conv(ctx, ctx->g_enc[i], enc_conv_layer(i, C), false)) return 1;
        // ... and layer 1 for the LDS-tiled kernel (generic_enc.hip): lane (co = lane & 31, h = lane >> 5) holds its two K operands of a tap
        const HostTensor* w = need(ctx, "down.qs_net.0.weight", {32, C, 3, 3});
        if (!w) return 1;
        std::vector<float> p1(9 * 64 * 2, 0.f);
        for (int t = 0; t < 9; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int i = 0; i < 2; ++i) {
                    const int co = lane & 31, ci = 2 * i + (lane >> 5);
                    if (ci < C) p1[(t * 64 + lane) * 2 + i] = w->data[((size_t)co * C + ci) * 9 + t];
                }
        if (!(ctx->g_enc1p = upload(ctx, p1))) return 1;
    } else {                // Dynamic-dSprites (1 x 64 x 64), the fused trunk: conv1 (Cin = 1) runs on the VALU: w1[tap][co]
        const WB t1 = weight_and_bias(ctx, "down.qs_net.0", {32, 1, 3, 3}, {32});
        if (!t1) return 1;
        std::vector<float> w1(288);
        for (int t = 0; t < 9; ++t) for (int co = 0; co < 32; ++co) w1[t * 32 + co] = t1.W()[co * 9 + t];
        if (!(ctx->enc_w1 = upload(ctx, w1)) || !(ctx->enc_b1 = upload(ctx, t1.b->data))) return 1;
        for (int i = 0; i < 2; ++i) if (pack_conv(ctx, ctx->enc_conv[i], enc_conv_layer(i + 1, 1), false)) return 1;
        // conv4 runs on v_mfma_f32_16x16x4_f32 (its 9 output pixels fill 9/16 of that tile, 9/32 of the 32-wide one):
        // [tap][16-channel block of Cin][16-channel tile of Cout][lane = (m, q)][s] = W[16 mt + m][16 blk + 4 q + s][tap]
        const WB t4 = weight_and_bias(ctx, "down.qs_net.6", {64, 64, 3, 3}, {64});
        if (!t4) return 1;
        std::vector<float> p((size_t)9 * 4 * 4 * 256);
        for (int t = 0; t < 9; ++t) for (int blk = 0; blk < 4; ++blk) for (int mt = 0; mt < 4; ++mt) for (int lane = 0; lane < 64; ++lane)
            for (int s_ = 0; s_ < 4; ++s_)
                p[((((size_t)t * 4 + blk) * 4 + mt) * 64 + lane) * 4 + s_] = t4.W()[((size_t)(16 * mt + (lane & 15)) * 64 + 16 * blk + 4 * (lane >> 4) + s_) * 9 + t];
        if (upload_layer(ctx, ctx->enc_conv[2], 9, 64, 64, p, t4.B())) return 1;
    }
    // Flatten is channel-major c*F + p (torchmodel.py:93); the last convolution's output is NHWC p*64 + c
    const std::vector<int> colp = nhwc_perm(64, F);
    const LayerSpec fc0{"down.qs_net.9", 256, F * 64};
    if (pack_linear(ctx, ctx->enc_fc[0], fc0, nullptr, colp.data()) || pack_linear16(ctx, ctx->enc16, 0, fc0, colp.data())) return 1;
    ctx->enc16_kc0 = F * 4;
    return 0;
}
// decoder (torchmodel.py:106-128) behind its head: Linear(256, 64 B^2), three ConvTranspose2d ([Cin][Cout][kh][kw]) and the final convolution
static int pack_decoder(efe_ctx* ctx) {
    const int C = ctx->chan, B = ctx->base;
    ctx->dec_raw = ctx->dect_raw = nullptr;
    if (C == 1 && ctx->res == 64) {     // the raw copy the backward passes read (train_dec_head.hip, train_dec.hip), beside the packed forward forms
        std::vector<float> flat;
        for (int i = 0; i < 4; ++i) {
            const LayerSpec s = i < 3 ? DEC_HEAD[i] : LayerSpec{"down.po_net.9", 16384, 256};
            const WB t = weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (flat.size() != (size_t)DEC_HEAD_P) return ctx->fail("decoder head: unexpected parameter count");
        for (int i = 0; i < 4; ++i) {
            const LayerSpec s = i < 3 ? DEC_CT[i] : LayerSpec{"down.po_net.19", 1, 32};
            const WB t = weight_and_bias(ctx, s.key, {s.in, s.out, 3, 3}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (flat.size() != (size_t)DEC_P) return ctx->fail("decoder tail: unexpected parameter count");
        if (!(ctx->dec_raw = upload_master(ctx, flat, ENC_P))) return 1;
        ctx->dect_raw = ctx->dec_raw + DEC_HEAD_P;
    }
    {   // Unflatten(1, (64, B, B)) is channel-major c*B*B + p (torchmodel.py:119); the layer emits NHWC p*64 + c directly
        const std::vector<int> rowp = nhwc_perm(64, B * B);
        if (pack_linear(ctx, ctx->generic ? ctx->g_fc4 : ctx->dec_fc[3], LayerSpec{"down.po_net.9", B * B * 64, 256}, rowp.data())) return 1;
    }
    const WB tf = weight_and_bias(ctx, "down.po_net.19", {32, C, 3, 3}, {C});
    if (!tf) return 1;
    if (ctx->generic) {
        for (int i = 0; i < 3; ++i) if (pack_conv(ctx, ctx->g_ct[i], DEC_CT[i], true)) return 1;
        std::vector<float> wf(9 * 32 * 4, 0.f);         // [tap][ci][c padded to 4]
        for (int t = 0; t < 9; ++t) for (int ci = 0; ci < 32; ++ci) for (int c = 0; c < C; ++c) wf[(t * 32 + ci) * 4 + c] = tf.W()[((size_t)ci * C + c) * 9 + t];
        if (!(ctx->g_wf = upload(ctx, wf))) return 1;
        for (int c = 0; c < 4; ++c) ctx->g_bf[c] = c < C ? tf.B()[c] : 0.f;
        return 0;
    }
    if (ctx->mfma_bf16x3 && pack_fc4_b3(ctx, (int)ctx->mfma_bf16x3)) return 1;
    for (int i = 0; i < 3; ++i) {
        const LayerSpec& s = DEC_CT[i];
        const WB t = weight_and_bias(ctx, s.key, {s.in, s.out, 3, 3}, {s.out});
        if (!t) return 1;
        if (i == 0) {       // po_net.13 (k_dec_a's layer 1): the 16 Winograd matrices as taps of the 32x32x2 form
            const std::vector<float> U = convt_s1_wino_weights(t.W(), s.in, s.out);
            if (upload_packed(ctx, ctx->dec_ct[0], 16, s.out, s.in, [&](int m, int co, int ci) { return U[((size_t)m * s.out + co) * s.in + ci]; }, t.B())) return 1;
        } else {            // po_net.15 (layer 2 of k_dec_a / k_dec_a_s, decoder.hip f22_l2) and po_net.17 (k_dec_b4's ConvT3): the 16 F(2, 2) matrices
            if (upload_layer(ctx, ctx->dec_ct[i], 16, s.out, s.in, pack_u16x16x4(convt_s2_f22_weights(t.W(), s.in, s.out), s.out), t.B())) return 1;
        }
    }
    std::vector<float> wf(288);                         // [tap][ci]
    for (int t = 0; t < 9; ++t) for (int ci = 0; ci < 32; ++ci) wf[t * 32 + ci] = tf.W()[ci * 9 + t];
    if (!(ctx->dec_wf = upload(ctx, wf))) return 1;
    ctx->dec_bf = tf.B()[0]; ctx->dec_bf_stale = false;
    return 0;
}

int efe_commit_weights(efe_ctx* ctx) {
    Call call(ctx, Mode::device); if (!call) return 1;
    // a re-commit replaces the packed buffers of the previous one: wait for work that may still read them, then free them
    if (!ctx->wbufs.empty()) {
        HIPCHK(hipDeviceSynchronize());
        for (void* p : ctx->wbufs) (void)hipFree(p);
        ctx->wbufs.clear();
        ctx->fc4_b3 = nullptr; ctx->ct_b3[0] = ctx->ct_b3[1] = nullptr; ctx->ct3_b3 = nullptr; ctx->split_packed = 0;
        ctx->dec_raw = ctx->dect_raw = ctx->enc_raw = nullptr;
    }
    ctx->committed = false;
    // a trained part is never reverted, whichever tensor the caller replaced: the host copies follow the device master copies first
    if (refresh_train_host(ctx, ctx->top_train) || refresh_train_host(ctx, ctx->mid_train) || refresh_down_host(ctx)) return 1;
    if (pack_top(ctx) || pack_mid(ctx) || pack_heads(ctx) || pack_encoder(ctx) || pack_decoder(ctx)) return 1;
    ctx->down_repack_n = 0;
    if (!ctx->generic && ctx->enc_raw && ctx->dec_raw && build_down_repack(ctx)) return 1;
    // the host copies stay: a caller may update a single tensor with efe_set_weight and commit again
    ctx->committed = true;
    return 0;
}

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

// ---- agent control state (csrc/agent.hip): every refusal comes before the first launch and names its entry point ----
static int agent_state(efe_ctx* ctx, const char* fn, const efe_agent* ag, AgentState& o) {
    if (!ag) return ctx->fail(std::string(fn) + ": agent is NULL");
    if (ag->E < 1) return ctx->fail(std::string(fn) + ": E < 1");
    if (ag->cap < 1) return ctx->fail(std::string(fn) + ": cap < 1");
    if (!ag->queue || !ag->head || !ag->len || !ag->crossings || !ag->reward_sum) return ctx->fail(std::string(fn) + ": a NULL array in efe_agent");
    o = AgentState{ag->queue, ag->head, ag->len, ag->crossings, ag->reward_sum, ag->E, ag->cap};
    return 0;
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

// the bodies of efe_encoder[_rows] and efe_rollout[_rows] (behind row_set, below); `who` = the entry point the caller used
static int encoder_call(efe_ctx* ctx, const char* who, const float* o, int M, const efe_noise* nz, const float* eps, const efe_rows* rows, float* s,
                        float* mean, float* logvar, void* stream);
static int rollout_call(efe_ctx* ctx, const char* who, const float* o, const float* pi, int M, int steps, int samples, int calc_mean, int per_stage_mean,
                        const efe_noise* nz, const float* eps, const efe_rows* rows, float* sum_G, float* sum_terms, float* po1, void* stream);
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

// ---- training of the habit net and the transition net (train.hip) -------------------------------------
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
extern "C++" template <class Launch>      // (a template inside the C ABI block)
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
}  // namespace

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

namespace {
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
}  // namespace

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

namespace {
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
}  // namespace

int efe_train_mid(efe_ctx* ctx, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp,
                  void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (train_mid_run(ctx, "efe_train_mid", s0, pi0, qs1_mean, qs1_logvar, M, params, nz, ps1_mean, ps1_logvar, F_mid, exp_avg, exp_avg_sq, hp, st)) return 1;
    return call.finish();
}

// ---- backward of the reconstruction loss through the decoder: ConvT tail (train_dec.hip), optionally behind the dense head (train_dec_head.hip) ----
namespace {
// the dense head's side of the call: its input, the keys of its four dropout masks, its outputs (all nullable but s and nz)
struct DecHeadIO { const float* s; const efe_noise* nz; float* d_s; float *h1, *h2, *h3, *h4; };

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
    const std::string w(who);
    if (M <= 0) return ctx->fail(w + ": M must be >= 1");
    if (!(hd ? hd->s && hd->nz : h4 != nullptr) || !o1 || !nlogpo1 || !grad)
        return ctx->fail(w + (hd ? ": s, o1, nz, nlogpo1 and grad must be non-NULL" : ": h4, o1, nlogpo1 and grad must be non-NULL"));
    if (ctx->chan != 1 || ctx->res != 64 || !(hd ? ctx->dec_raw : ctx->dect_raw)) return ctx->fail(w + ": built for the 1 x 64 x 64 geometry only");
    if (ctx->mfma_bf16x3) return ctx->fail(w + ": not available with the split-operand options (mfma_bf16x3 / mfma_f16x2) on");
    if (!(scale >= 0.0f)) {
        if (!(scale < 0.0f) || !std::isfinite(beta_o)) return ctx->fail(w + ": scale is NaN, or negative (= beta_o / M) with a non-finite beta_o");
        scale = beta_o / (float)M;
    }
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
}  // namespace

int efe_dec_tail_grad(efe_ctx* ctx, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1, float* po1, float* d_h4,
                      float* grad, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (dec_grad(ctx, "efe_dec_tail_grad", nullptr, h4, d_h4, o1, M, scale, beta_o, nlogpo1, po1, grad, y1, y2, y3, st)) return 1;
    return call.finish();
}

int efe_dec_grad(efe_ctx* ctx, const float* s, const float* o1, int M, float scale, float beta_o, const efe_noise* nz, float* nlogpo1, float* po1,
                 float* d_s, float* grad, float* h1, float* h2, float* h3, float* h4, float* y1, float* y2, float* y3, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    const DecHeadIO hd{s, nz, d_s, h1, h2, h3, h4};
    if (dec_grad(ctx, "efe_dec_grad", &hd, nullptr, nullptr, o1, M, scale, beta_o, nlogpo1, po1, grad, y1, y2, y3, st)) return 1;
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

namespace {
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
}  // namespace

int efe_down_grad(efe_ctx* ctx, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return 1;
    if (down_grad_run(ctx, "efe_down_grad", o1, ps1_mean, ps1_logvar, M, params, nz, eps, out, g_mean, g_logvar, grad, st)) return 1;
    return call.finish();
}

namespace {
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
}  // namespace

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

int efe_down_get_weights(efe_ctx* ctx, float* dst, int64_t n, void* stream) {
    hipStream_t st = (hipStream_t)stream; Call call(ctx, Mode::scratch, st); if (!call) return call.refused("efe_down_get_weights");
    if (ctx->chan != 1 || ctx->res != 64 || !ctx->down_master) return ctx->fail("efe_down_get_weights: built for the 1 x 64 x 64 geometry only");
    if (!dst || n != DOWN_P) return ctx->fail("efe_down_get_weights: dst must hold efe_param_count(\"down\") floats");
    HIPCHK(hipMemcpyAsync(dst, ctx->down_master, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return call.finish();
}

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

// ---- EFE level -----------------------------------------------------------------------------------------
// the row set of a call (efe_rows; NULL = every row, identity)
struct RowSet { const uint8_t* mask; const int32_t* ids; int div; };
static int row_set(efe_ctx* ctx, const efe_rows* rows, int n_rows, int fixed_div, RowSet& out, const char* who, hipStream_t st) {
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

// the noise of the single-group pass (pass, sample) of a call over the row set rs (rows == NULL: exactly pass_noise)
static NoiseCfg pass_noise_rows(const efe_noise* nz, uint32_t pass, uint32_t sample, int M, const efe_rows* rows, const RowSet& rs) {
    if (!rows) return pass_noise(nz, pass, sample, M);
    return make_noise((uint32_t)nz->seed, (uint32_t)(nz->seed >> 32), M, nz->row_offset, GroupMap{1, 1, {pass, 0, 0}, nz->stage, sample}, rs.ids, rs.div, rs.mask);
}

// `who`: the entry point the caller used; every refusal names it
static int encoder_call(efe_ctx* ctx, const char* who, const float* o, int M, const efe_noise* nz, const float* eps, const efe_rows* rows, float* s,
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

static int rollout_call(efe_ctx* ctx, const char* who, const float* o, const float* pi, int M, int steps, int samples, int calc_mean, int per_stage_mean,
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

static int trajectory_impl(efe_ctx* ctx, const float* s0_traj, const float* ps1_traj, const float* mean_traj, const float* lv_traj,
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
