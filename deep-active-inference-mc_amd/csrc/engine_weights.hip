// Host side of the engine, the weights: the host tensors a caller sets (efe_set_weight) packed into every device form the kernels read
// (efe_commit_weights), the training tables of the trainable parts, and the way back from a device-side optimiser step to the host tensors.
#include "engine.h"

namespace efe {
namespace host {
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

// ... of the master copy of a generic context (owned, allocated at the first commit: the geometry, and with it the length, is the context's)
float* upload_master_g(efe_ctx* ctx, const std::vector<float>& v, size_t off) {
    const size_t P = (size_t)down_g_count(ctx);
    if (off + v.size() > P) { ctx->err = "master copy: a span past the parameter count"; return nullptr; }
    if (!ctx->down_master_g) {
        if (hipMalloc((void**)&ctx->down_master_g, P * 4) != hipSuccess) { ctx->err = "master copy: hipMalloc failed"; return nullptr; }
        ctx->owned.push_back(ctx->down_master_g);
    }
    if (hipMemcpy(ctx->down_master_g + off, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "master copy: hipMemcpy failed"; return nullptr; }
    return ctx->down_master_g + off;
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
const char* const TOP_KEYS[TOP_NL] = {"top.qpi_net.0", "top.qpi_net.2", "top.qpi_net.4"};
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

// The table a repack kernel works from: one entry per packed buffer and bias table, with the buffers of THIS commit; the kinds name the
// packers they invert.  blocks: the first workgroup of the next entry (256 owning threads each).
struct RepackTable {
    std::vector<RepackDesc> t;
    int64_t blocks = 0;
    void add(float* dst, int64_t src, int kind, int64_t n, int out, int in, int KC, int mtiles, int row_ch = 0, int row_pos = 0, int col_ch = 0, int col_pos = 0) {
        RepackDesc d{};
        d.dst = dst; d.src = (int)src; d.kind = kind; d.n = (int)n; d.block0 = (int)blocks; d.out = out; d.in = in; d.KC = KC; d.mtiles = mtiles;
        d.row_ch = row_ch; d.row_pos = row_pos; d.col_ch = col_ch; d.col_pos = col_pos;
        d.vec = (kind == RP_DENSE32 || kind == RP_DENSE16) && !col_ch && src % 4 == 0 && in % (kind == RP_DENSE32 ? 8 : 16) == 0;
        d.swizzle = kind == RP_DENSE32 && d.vec && KC % 4 == 0;
        if (src > INT32_MAX || n > INT32_MAX) fits = false;
        blocks += (n + 255) / 256;
        t.push_back(d);
    }
    bool fits = true;       // every offset, thread count and first block is an int of the device table
    void bias(float* dst, int64_t src, int out, int n, int row_ch = 0, int row_pos = 0) { add(dst, src, RP_BIAS, n, out, 0, 0, 0, row_ch, row_pos); }
    void dense32(const Layer& L, int64_t w, int64_t b, int out, int in, int row_ch = 0, int row_pos = 0, int col_ch = 0, int col_pos = 0) {
        add(L.Wp, w, RP_DENSE32, (int64_t)L.mtiles * (L.cin / 8) * 64, out, in, L.cin / 8, L.mtiles, row_ch, row_pos, col_ch, col_pos);
        bias(L.bias, b, out, L.mtiles * 32, row_ch, row_pos);
    }
    void dense16(const MlpW& net, int layer, int64_t w, int64_t b, int out, int in, int col_ch = 0, int col_pos = 0) {
        const int mtiles = (out + 15) / 16, KC = (in + 15) / 16;
        add(const_cast<float*>(reinterpret_cast<const float*>(net.w[layer])), w, RP_DENSE16, (int64_t)mtiles * KC * 64, out, in, KC, mtiles, 0, 0, col_ch, col_pos);
        bias(const_cast<float*>(net.b[layer]), b, out, mtiles * 16);
    }
    // a conv layer of nine taps in the 32x32x2 form (RP_CONV32 / RP_CONVT32) and its bias
    void conv32(const Layer& L, int kind, int64_t w, int64_t b, int out, int in) {
        add(L.Wp, w, kind, (int64_t)9 * L.mtiles * (L.cin / 8) * 64, out, in, L.cin / 8, L.mtiles);
        bias(L.bias, b, out, L.mtiles * 32);
    }
    // checked and copied into the context's device table (owned, allocated once)
    int commit(efe_ctx* ctx, RepackDesc*& dev, int& n, int& nblocks) const {
        constexpr size_t CAP = 64;
        if (t.size() > CAP) return ctx->fail("repack table: more entries than its buffer holds");
        for (const RepackDesc& d : t) if (!d.dst) return ctx->fail("repack table: a packed buffer is missing");
        if (!fits || blocks > INT32_MAX) return ctx->fail("repack table: an offset or a thread count does not fit the table's ints");
        if (!dev) {
            HIPCHK(hipMalloc((void**)&dev, CAP * sizeof(RepackDesc))); ctx->owned.push_back(dev);
        }
        HIPCHK(hipMemcpy(dev, t.data(), t.size() * sizeof(RepackDesc), hipMemcpyHostToDevice));
        n = (int)t.size(); nblocks = (int)blocks;
        return 0;
    }
};

// the table k_repack_down works from (train_down.hip): pack_heads, pack_encoder and pack_decoder on the 1 x 64 x 64 path
int build_down_repack(efe_ctx* ctx) {
    RepackTable tb;
    const int D = ENC_P, T = ENC_P + DEC_HEAD_P;      // po_net and its ConvT tail inside the master copy
    // pack_heads
    const int dh[3][4] = {{DH_W0, DH_B0, 256, 10}, {DH_W1, DH_B1, 256, 256}, {DH_W2, DH_B2, 256, 256}};
    const int eh[3][4] = {{EQ_W12, EQ_B12, 256, 256}, {EQ_W15, EQ_B15, 256, 256}, {EQ_W18, EQ_B18, 20, 256}};
    for (int i = 0; i < 3; ++i) {
        tb.dense32(ctx->dec_fc[i], D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]); tb.dense16(ctx->dec16, i, D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]);
        tb.dense32(ctx->enc_fc[i + 1], eh[i][0], eh[i][1], eh[i][2], eh[i][3]); tb.dense16(ctx->enc16, i + 1, eh[i][0], eh[i][1], eh[i][2], eh[i][3]);
    }
    // pack_encoder: conv1 on the VALU, conv2 / conv3 as nine taps of the 32x32x2 form, conv4 in the 16x16x4 form, the head's first layer (columns NHWC)
    tb.add(ctx->enc_w1, EQ_W1, RP_TAP32, 288, 32, 1, 0, 0); tb.bias(ctx->enc_b1, EQ_B1, 32, 32);
    tb.add(ctx->enc_conv[0].Wp, EQ_W2, RP_CONV32, 9 * 1 * 4 * 64, 32, 32, 4, 1); tb.bias(ctx->enc_conv[0].bias, EQ_B2, 32, 32);
    tb.add(ctx->enc_conv[1].Wp, EQ_W3, RP_CONV32, 9 * 2 * 4 * 64, 64, 32, 4, 2); tb.bias(ctx->enc_conv[1].bias, EQ_B3, 64, 64);
    tb.add(ctx->enc_conv[2].Wp, EQ_W4, RP_CONV16, 9 * 4 * 4 * 64, 64, 64, 4, 4); tb.bias(ctx->enc_conv[2].bias, EQ_B4, 64, 64);
    tb.dense32(ctx->enc_fc[0], EQ_W9, EQ_B9, 256, 576, 0, 0, 64, 9); tb.dense16(ctx->enc16, 0, EQ_W9, EQ_B9, 256, 576, 64, 9);
    // pack_decoder: Linear(256, 16384) with its rows NHWC, the Winograd and F(2, 2) matrices, the final convolution (its bias: ctx->dec_bf)
    tb.dense32(ctx->dec_fc[3], D + DH_W3, D + DH_B3, 16384, 256, 64, 256);
    tb.add(ctx->dec_ct[0].Wp, T + DT_W1, RP_WINO, 16 * 2 * 8 * 64, 64, 64, 8, 2); tb.bias(ctx->dec_ct[0].bias, T + DT_B1, 64, 64);
    tb.add(ctx->dec_ct[1].Wp, T + DT_W2, RP_F22, 16 * 4 * 4 * 64, 64, 64, 4, 4); tb.bias(ctx->dec_ct[1].bias, T + DT_B2, 64, 64);
    tb.add(ctx->dec_ct[2].Wp, T + DT_W3, RP_F22, 16 * 2 * 4 * 64, 32, 64, 4, 2); tb.bias(ctx->dec_ct[2].bias, T + DT_B3, 32, 32);
    tb.add(ctx->dec_wf, T + DT_W4, RP_TAP32, 288, 32, 1, 0, 0);
    return tb.commit(ctx, ctx->down_repack, ctx->down_repack_n, ctx->down_repack_blocks);
}

// the table k_repack_down_g works from (train_down_g.hip): the same three packers under ctx->generic, offsets from the context's geometry.
// Largest geometry (3 x 128 x 128): 18.0 M floats of master copy, 4.2 M owning threads for g_fc4, 17 K workgroups: RepackTable::commit
// checks that each fits an int.
int build_down_repack_g(efe_ctx* ctx) {
    RepackTable tb;
    const int C = ctx->chan, B = ctx->base, F4 = ctx->enc_hw[4] * ctx->enc_hw[4];
    const EncGeo eg{C, ctx->res};
    const DecHeadGeo hg{B};
    const int64_t S = eg.small(), D = eg.P(), T = D + (int64_t)hg.P();      // qs_net.12 ..; po_net; its ConvT tail, inside the master copy
    // pack_heads
    const int dh[3][4] = {{DH_W0, DH_B0, 256, 10}, {DH_W1, DH_B1, 256, 256}, {DH_W2, DH_B2, 256, 256}};
    const int eh[3][4] = {{EQS_W12, EQS_B12, 256, 256}, {EQS_W15, EQS_B15, 256, 256}, {EQS_W18, EQS_B18, 20, 256}};
    for (int i = 0; i < 3; ++i) {
        tb.dense32(ctx->dec_fc[i], D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]); tb.dense16(ctx->dec16, i, D + dh[i][0], D + dh[i][1], dh[i][2], dh[i][3]);
        tb.dense32(ctx->enc_fc[i + 1], S + eh[i][0], S + eh[i][1], eh[i][2], eh[i][3]); tb.dense16(ctx->enc16, i + 1, S + eh[i][0], S + eh[i][1], eh[i][2], eh[i][3]);
    }
    // pack_encoder: four k_conv_g layers (layer 0 reads C channels, padded to 8), layer 1 again for the LDS-tiled kernels, the head's first layer (columns NHWC)
    const int ew[4] = {eg.w1(), eg.w2(), eg.w3(), eg.w4()}, eb[4] = {eg.b1(), eg.b2(), eg.b3(), eg.b4()};
    for (int i = 0; i < 4; ++i) { const LayerSpec s = enc_conv_layer(i, C); tb.conv32(ctx->g_enc[i], RP_CONV32, ew[i], eb[i], s.out, s.in); }
    tb.add(ctx->g_enc1p, eg.w1(), RP_ENC1P, 9 * 64 * 2, 32, C, 0, 0);
    tb.dense32(ctx->enc_fc[0], eg.w9(), eg.b9(), 256, eg.K(), 0, 0, 64, F4); tb.dense16(ctx->enc16, 0, eg.w9(), eg.b9(), 256, eg.K(), 64, F4);
    // pack_decoder: Linear(256, 64 B^2) with its rows NHWC, three transposed convolutions, the final convolution (its bias: ctx->g_bf)
    tb.dense32(ctx->g_fc4, D + DH_W3, D + (int64_t)hg.b3(), hg.F(), 256, 64, B * B);
    const int tw[3] = {DT_W1, DT_W2, DT_W3}, tbs[3] = {DT_B1, DT_B2, DT_B3};
    for (int i = 0; i < 3; ++i) tb.conv32(ctx->g_ct[i], RP_CONVT32, T + tw[i], T + tbs[i], DEC_CT[i].out, DEC_CT[i].in);
    tb.add(ctx->g_wf, T + DT_W4, RP_WF4, 9 * 32 * 4, C, 32, 0, 0);
    return tb.commit(ctx, ctx->down_repack_g, ctx->down_repack_g_n, ctx->down_repack_g_blocks);
}

// the split-operand planes of pack_fc4_b3, released
void drop_split_planes(efe_ctx* ctx) {
    void* old[4] = {ctx->fc4_b3, ctx->ct_b3[0], ctx->ct_b3[1], ctx->ct3_b3};
    for (void* q : old) {
        if (!q) continue;
        ctx->wbufs.erase(std::remove(ctx->wbufs.begin(), ctx->wbufs.end(), q), ctx->wbufs.end());
        (void)hipFree(q);
    }
    ctx->fc4_b3 = nullptr; ctx->ct_b3[0] = ctx->ct_b3[1] = nullptr; ctx->ct3_b3 = nullptr; ctx->split_packed = 0;
}

// a dense net in both packed forms: 32x32x2 tiles for k_dense (the layer-by-layer path) and 16x16x4 tiles for the fused kernels
int pack_net(efe_ctx* ctx, int nl, LayerSpec (*layer)(int, int), Layer* L32, MlpW& L16) {
    for (int i = 0; i < nl; ++i) {
        const LayerSpec s = layer(i, ctx->pi_dim);
        if (pack_linear(ctx, L32[i], s) || pack_linear16(ctx, L16, i, s)) return 1;
    }
    return 0;
}
int pack_top(efe_ctx* ctx) { return pack_net(ctx, TOP_NL, top_layer, ctx->top, ctx->top16) || build_top_train(ctx); }
int pack_mid(efe_ctx* ctx) { return pack_net(ctx, MID_NL, mid_layer, ctx->mid, ctx->mid16) || build_mid_train(ctx); }
// the geometry-independent dense layers of the decoder / encoder heads (the encoder's first layer: pack_encoder)
int pack_heads(efe_ctx* ctx) {
    for (int i = 0; i < 3; ++i) {
        if (pack_linear(ctx, ctx->dec_fc[i], DEC_HEAD[i]) || pack_linear16(ctx, ctx->dec16, i, DEC_HEAD[i])) return 1;
        if (pack_linear(ctx, ctx->enc_fc[i + 1], ENC_HEAD[i]) || pack_linear16(ctx, ctx->enc16, i + 1, ENC_HEAD[i])) return 1;
    }
    return 0;
}
// encoder (torchmodel.py:84-104): the convolution stack, then the head's first layer
int pack_encoder(efe_ctx* ctx) {
    const int C = ctx->chan, F = ctx->enc_hw[4] * ctx->enc_hw[4];
    ctx->enc_raw = ctx->enc_raw_g = nullptr;
    {   // the raw copy the training forward and backward read (train_enc.hip, train_enc_g.hip), beside the packed forward forms
        const EncGeo eg{C, ctx->res};
        std::vector<float> flat;
        flat.reserve((size_t)eg.P());
        for (int i = 0; i < 8; ++i) {
            const LayerSpec s = i < 4 ? enc_conv_layer(i, C) : i == 4 ? LayerSpec{"down.qs_net.9", 256, F * 64} : ENC_HEAD[i - 5];
            const WB t = i < 4 ? weight_and_bias(ctx, s.key, {s.out, s.in, 3, 3}, {s.out}) : weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (F * 64 != eg.K() || flat.size() != (size_t)eg.P()) return ctx->fail("encoder: unexpected parameter count");
        if (C == 1 && ctx->res == 64) {     // inside ModelDown's master vector, so that it follows an optimiser step
            if (flat.size() != (size_t)ENC_P) return ctx->fail("encoder: unexpected parameter count");
            if (!(ctx->enc_raw = upload_master(ctx, flat, 0))) return 1;
            ctx->enc_raw_g = ctx->enc_raw;
        } else {                            // any other geometry: the head of that context's master copy; po_net behind it stays 16-byte aligned
            if (eg.P() % 4) return ctx->fail("encoder: the parameter count is no multiple of 4 floats (the decoder's span of the master copy would be misaligned)");
            if (!(ctx->enc_raw_g = upload_master_g(ctx, flat, 0))) return 1;
        }
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
int pack_decoder(efe_ctx* ctx) {
    const int C = ctx->chan, B = ctx->base;
    ctx->dec_raw = ctx->dect_raw = ctx->dec_raw_g = ctx->dect_raw_g = nullptr;
    {   // the raw copy the backward passes read, beside the packed forward forms: the whole po_net flat in parameters() order
        const DecHeadGeo hg{B};
        const size_t tail = (size_t)DT_W4 + 289 * (size_t)C;
        std::vector<float> flat;
        flat.reserve(hg.P() + tail);
        for (int i = 0; i < 4; ++i) {
            const LayerSpec s = i < 3 ? DEC_HEAD[i] : LayerSpec{"down.po_net.9", hg.F(), 256};
            const WB t = weight_and_bias(ctx, s.key, {s.out, s.in}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (flat.size() != hg.P()) return ctx->fail("decoder head: unexpected parameter count");
        for (int i = 0; i < 4; ++i) {
            const LayerSpec s = i < 3 ? DEC_CT[i] : LayerSpec{"down.po_net.19", C, 32};
            const WB t = weight_and_bias(ctx, s.key, {s.in, s.out, 3, 3}, {s.out});
            if (!t) return 1;
            flat.insert(flat.end(), t.w->data.begin(), t.w->data.end());
            flat.insert(flat.end(), t.b->data.begin(), t.b->data.end());
        }
        if (flat.size() != hg.P() + tail) return ctx->fail("decoder tail: unexpected parameter count");
        if (C == 1 && ctx->res == 64) {     // inside ModelDown's master vector, so that it follows an optimiser step (train_dec_head.hip, train_dec.hip)
            if (!(ctx->dec_raw = upload_master(ctx, flat, ENC_P))) return 1;
            ctx->dec_raw_g = ctx->dec_raw;
            ctx->dect_raw = ctx->dec_raw + DEC_HEAD_P;
        } else if (!(ctx->dec_raw_g = upload_master_g(ctx, flat, (size_t)EncGeo{C, ctx->res}.P()))) return 1;      // any other geometry: behind qs_net in that context's master copy (train_dec_head_g.hip, train_dec_g.hip)
        ctx->dect_raw_g = ctx->dec_raw_g + hg.P();
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
        ctx->g_bf_stale = false;
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

}  // namespace

// ---- what other host files call (engine.h) -----------------------------------------------------------
// habit net (torchmodel.py:19-25)
LayerSpec top_layer(int i, int A) { const int out[TOP_NL] = {128, 128, A}, in[TOP_NL] = {10, 128, 128}; return {TOP_KEYS[i], out[i], in[i]}; }
// transition net (torchmodel.py:41-52); input = cat[pi, s0] (torchmodel.py:59)
LayerSpec mid_layer(int i, int A) {
    const LayerSpec t[MID_NL] = {{"mid.ps_net.0", 512, A + 10}, {"mid.ps_net.3", 512, 512}, {"mid.ps_net.6", 512, 512}, {"mid.ps_net.9", 20, 512}};
    return t[i];
}
int part_param_count(int nl, LayerSpec (*layer)(int, int), int A) { int n = 0; for (int i = 0; i < nl; ++i) { const LayerSpec s = layer(i, A); n += s.out * s.in + s.out; } return n; }

int64_t down_g_count(const efe_ctx* ctx) {
    return (int64_t)EncGeo{ctx->chan, ctx->res}.P() + (int64_t)DecHeadGeo{ctx->base}.P() + DecTailGeo{ctx->base, ctx->chan, ctx->last_s1 ? 1 : 2}.P();
}

// refresh_train_host for ModelDown's master copy, over DOWN_KEYS: down_master at 1 x 64 x 64, down_master_g on a generic context (the
// sizes are the host tensors' own; their sum is held to the geometry's parameter count)
int refresh_down_host(efe_ctx* ctx) {
    if (!ctx->down_dirty) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    const float* master = ctx->generic ? ctx->down_master_g : ctx->down_master;
    if (!master) return ctx->fail("master copy: marked newer than the host tensors, but never allocated");
    std::vector<float> flat((size_t)(ctx->generic ? down_g_count(ctx) : DOWN_P));
    HIPCHK(hipMemcpy(flat.data(), master, flat.size() * 4, hipMemcpyDeviceToHost));
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
    if (ctx->generic) {     // po_net.19.bias, the vector's last chan floats
        for (int c = 0; c < 4; ++c) ctx->g_bf[c] = c < ctx->chan ? flat[flat.size() - (size_t)ctx->chan + c] : 0.f;
        ctx->g_bf_stale = false;
    } else { ctx->dec_bf = flat.back(); ctx->dec_bf_stale = false; }
    ctx->down_dirty = false;
    return 0;
}

// options mfma_bf16x3 (mode 1) / mfma_f16x2 (mode 2): po_net.9 (rows in NHWC order), po_net.13 / .15 / .17 as 16-bit planes for the kernels of
// bf16x3.hip.  Planes of the other mode are released first; a failure leaves no planes at all.
int pack_fc4_b3(efe_ctx* ctx, int mode) {
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

}  // namespace host
}  // namespace efe

extern "C" {

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

int efe_commit_weights(efe_ctx* ctx) {
    Call call(ctx, Mode::device); if (!call) return 1;
    // a re-commit replaces the packed buffers of the previous one: wait for work that may still read them, then free them
    if (!ctx->wbufs.empty()) {
        HIPCHK(hipDeviceSynchronize());
        for (void* p : ctx->wbufs) (void)hipFree(p);
        ctx->wbufs.clear();
        ctx->fc4_b3 = nullptr; ctx->ct_b3[0] = ctx->ct_b3[1] = nullptr; ctx->ct3_b3 = nullptr; ctx->split_packed = 0;
        ctx->dec_raw = ctx->dect_raw = ctx->dec_raw_g = ctx->dect_raw_g = ctx->enc_raw = ctx->enc_raw_g = nullptr;
    }
    ctx->committed = false;
    // a trained part is never reverted, whichever tensor the caller replaced: the host copies follow the device master copies first
    if (refresh_train_host(ctx, ctx->top_train) || refresh_train_host(ctx, ctx->mid_train) || refresh_down_host(ctx)) return 1;
    if (pack_top(ctx) || pack_mid(ctx) || pack_heads(ctx) || pack_encoder(ctx) || pack_decoder(ctx)) return 1;
    ctx->down_repack_n = ctx->down_repack_g_n = 0;
    if (!ctx->generic && ctx->enc_raw && ctx->dec_raw && build_down_repack(ctx)) return 1;
    if (ctx->generic && build_down_repack_g(ctx)) return 1;
    // the host copies stay: a caller may update a single tensor with efe_set_weight and commit again
    ctx->committed = true;
    return 0;
}

}  // extern "C"
