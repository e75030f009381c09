// Device kernels of the EFE rollout engine (gfx950 / CDNA4 only): shared argument structs and launchers.
//
// Every dense contraction on the hot path (reference layers: /root/reference/src/torchmodel.py:41-52 ps_net,
// :84-104 qs_net, :106-128 po_net, :19-25 qpi_net) has the same MFMA mapping:
//
//   * MFMA rows  = output features (A operand = weights, pre-packed fragment-major so every wave-level load is one
//                  fully coalesced 1 KiB global_load_dwordx4),
//   * MFMA cols  = batch rows / output pixels (B operand = NHWC activations, 16 B per lane, from LDS in the fused
//                  kernels or straight from L2 in k_dense),
//   * v_mfma_f32_32x32x2_f32: exact fp32 (bitwise an fmaf chain), 64 FLOP/clk/SIMD,
//   * a lane owns ONE batch row / pixel and 16 features per 32x32 tile, so the MC-dropout mask of a row is one Philox
//     call per 128 features, generated in the epilogue; no mask is ever stored.
//
// kernels.hip: k_dense + the small VALU kernels (reparameterisation, term combine, softmax, sampling);
// decoder.hip: k_fc4, k_dec_a, k_dec_b;  encoder.hip: k_enc_trunk;  mfma_pipe.h: the shared software pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox.h"

namespace efe {

// The batch of one launch is [group][row]: a group is one network evaluation ("pass") over the same
// rows_per_group logical rows.  Group g of a multi-stage batch decomposes as t = g / per_stage (stage),
// q = g % per_stage, pass = pass[q / S], sample = sample0 + q % S.
struct GroupMap {
    int per_stage, S;
    uint32_t pass[3];
    uint32_t stage0, sample0;
    // optional row identities (efe_rows.ids: the lock-step planner's compacted batches): logical row r of a group is row
    // ids[r / ids_div] * ids_div + r % ids_div of the un-compacted batch -- the noise keys follow the episode, not its slot
    const int32_t* ids = nullptr; int ids_div = 1;
};
// global noise row of logical row r of a group (counter word 1 of every Philox draw of that row)
__device__ __forceinline__ uint32_t global_row(const int32_t* ids, int ids_div, int r, uint32_t row_offset) {
    if (!ids) return row_offset + (uint32_t)r;
    const int e = r / ids_div;
    return row_offset + (uint32_t)(ids[e] * ids_div + (r - e * ids_div));
}
__host__ __device__ inline void group_decode(const GroupMap& gm, int g, int& t, int& pidx, int& samp) {
    t = g / gm.per_stage;
    const int q = g - t * gm.per_stage;
    pidx = q / gm.S;
    samp = q - pidx * gm.S;
}
__device__ __forceinline__ uint2 group_key(const GroupMap& gm, int g) {
    int t, pidx, samp;
    group_decode(gm, g, t, pidx, samp);
    const uint32_t pass = pidx == 0 ? gm.pass[0] : pidx == 1 ? gm.pass[1] : gm.pass[2];
    return make_uint2(stream_id(pass, gm.sample0 + (uint32_t)samp), gm.stage0 + (uint32_t)t);
}

// Optional liveness mask of the logical rows of a call (efe_rows.mask: the lock-step planner's early-stopped episodes): image m of
// a launch belongs to logical row (m0 + m) % rows_per_group and is evaluated iff mask == nullptr or mask[row / div] != 0.  The
// per-image kernels (decoder stages, encoder trunk) skip dead images; the outputs of dead rows are unspecified.
struct RowMask {
    const uint8_t* mask; int div, m0, rows_per_group;
    const int32_t* ids = nullptr;       // optional: entry slot -> entry id (the mask is indexed by id)
};
__device__ __forceinline__ bool row_live(const RowMask& k, int m) {
    if (!k.mask) return true;
    const int slot = ((k.m0 + m) % k.rows_per_group) / k.div;
    return k.mask[k.ids ? k.ids[slot] : slot] != 0;
}

// Non-finite propagation ("Non-finite values"): the forms every layer epilogue and backward gate is written in.
//   relu_nan : torch's relu -- max(x, 0) that RETURNS a NaN x of either sign (fmaxf returns 0 for it, a signed-integer maximum of the bit
//              pattern 0 for a negative-signed one).  IEEE 754-2019 maximum: one v_maximum3_f32 on gfx950; -0 gives +0, finite values and
//              +inf keep every bit.
//   keep2    : the factor of a dropout mask, 2 for a kept unit and 0 for a dropped one.  The mask MULTIPLIES (h * mask, as F.dropout
//              does): a dropped NaN or inf unit stays NaN, which a select (keep ? 2 h : 0) would turn into 0.
//   gate_open: torch's threshold_backward zeroes the upstream gradient only where the stored activation is <= 0, so a NaN activation lets it
//              through (a > 0 test would zero it).
//   gated    : the gradient t behind a ReLU (and, `masked`, a dropout mask whose factor t already carries), read off the ONE stored
//              activation h = relu(x) [* mask].  Open gate: t.  Closed without a mask: exactly 0, as threshold_backward gives.  Closed behind a
//              mask, h = 0 is an inactive unit (torch: 0) or an active dropped one (torch: t * 0, NaN for a non-finite t) and the stored value
//              cannot tell which: t - t serves both -- +0 for every finite t (the same bits as the select), NaN for a non-finite one.  That
//              is a superset of torch's NaN set, inside rows whose upstream gradient is not finite already.
__device__ __forceinline__ float relu_nan(float x) { return __builtin_elementwise_maximum(x, 0.0f); }
__device__ __forceinline__ float keep2(bool keep) { return keep ? 2.0f : 0.0f; }
__device__ __forceinline__ bool gate_open(float a) { return !(a <= 0.0f); }
__device__ __forceinline__ float gated(float h, float t, bool relu, bool masked) {
#pragma clang fp contract(off)
    if (!relu || gate_open(h)) return t;
    return masked ? t - t : 0.0f;
}

// One pixel's term of the reward log-likelihood log_bernoulli(x = pr, p = target) (/root/reference/src/torchutils.py:30-37):
//   intent 0: what the shipped port computes -- on NCHW input the target broadcasts to 1 for image rows oh < H / 2 and 0 below, and
//             every pixel counts (pinned by the oracle);
//   intent 1: what the upstream NHWC code means -- only the top three rows (the reward bar) count, with target 1
//             on their left half and 0 on the right half.
__device__ __forceinline__ float reward_term(float pr, int oh, int ow, int H, int W, int intent) {
#pragma clang fp contract(off)
    const float D1 = 1.00001f, D0 = 0.00001f;
    const bool one = intent ? (ow < W / 2) : (oh < H / 2);
    // (explicit contraction: the same bits from every inlined copy)
    const float t = one ? __builtin_fmaf(pr, logf(D1), (1.0f - pr) * logf(D1 - 1.0f)) : __builtin_fmaf(pr, logf(D0), (1.0f - pr) * logf(D1));
    return (intent && oh >= 3) ? 0.0f : t;
}

struct GemmArgs {
    const float* Wp;      // packed weights [tap][mtile][kc][64 lanes][4]
    const float* bias;    // [mtiles*32]
    const float* X;       // input activations
    float* Y;             // output activations
    const float* zeros;   // >= 4 KiB of zeros (source for padded taps / out-of-range rows)
    int n_pix;            // GEMM columns in this launch (batch rows)
    int cin;              // K per tap (multiple of 8)
    int cout;             // real output features (multiple of 4)
    int mtiles;           // 32-feature tiles in the packed weights
    int ldx, ldy;         // row strides in floats
    int x_mod;            // if > 0 the input row is (m % x_mod)  (same input for every MC pass)
    int relu;
    // MC-dropout: keep-mask * 2.0 from Philox, keyed by (tag, global row, group key)
    int dropout;
    uint32_t tag, k0, k1;
    GroupMap gm;          // group index -> (stream id, stage)
    int rows_per_group;
    uint32_t row_offset;  // global index of row 0 of a group on this rank
    int m0;               // index of column 0 of this launch inside the [group][row] batch
    const void* Wb3 = nullptr;   // options mfma_bf16x3 / mfma_f16x2 (bf16x3.hip): the same weights as 16-bit planes [mtile][16][planes][64 lanes][8]
    int split = 0;               // 1 = three bf16 planes, 2 = two fp16 planes
    float wb3_scale_inv = 1.0f;  // fp16 split: 1 / (the power of two the packed weights were scaled by)
};

// fused decoder, stage A: x4 [rows][16][16][64] -> ConvT(64,64,s1)+ReLU -> ConvT(64,64,s2)+ReLU -> y2 [rows][4 parities][8 channel groups][16x16 positions][8] (see k_dec_a)
struct DecAArgs {
    const float* x4; float* y2;
    const float* w1; const float* b1;   // Winograd F(2x2,3x3) weights packed [16 xi][2][8][64][4] (decoder.hip wino_l1), bias [64]
    const float* w2; const float* b2;   // F(2, 2) weights packed [16 U][4 channel tiles][4 chunks][64][4] (engine_weights.hip; decoder.hip f22_l2), bias [64]
    int rows;
    RowMask live;
    int parts;            // 1 = persistent, one image per workgroup pass; 8 = small launches, an image over eight workgroups (k_dec_a_s)
    int* queue;           // zero-initialised ticket counter of this launch: images beyond the first two per workgroup are claimed dynamically
    const void* w1b3 = nullptr; const void* w2b3 = nullptr;      // options mfma_bf16x3 / mfma_f16x2: the two layers' weights as 16-bit planes [tap][2][4][planes][64 lanes][8] (bf16x3.hip)
    int split = 0;                                               // 1 = three bf16 planes, 2 = two fp16 planes
    float w1s = 1.0f, w1s_inv = 1.0f, w2s = 1.0f, w2s_inv = 1.0f;  // fp16 split: the layers' weight scales (powers of two) and their inverses
};
// fused decoder, stage B: y2 -> ConvT(64,32,s2)+ReLU -> ConvT(32,1,s1)+Sigmoid -> per-image reduction (+ image store)
// Minimal filtering F(2, 2) of a stride-2 transposed conv along one dimension (ConvTranspose2d(k 3, s 2, p 1, op 1), oh = 2 ih - 1 + kh;
// decoder.hip k_dec_b4): for the input pair block u, x0 = x[2u], x1 = x[2u + 1], x2 = x[2u + 2], the views d0 = x0 - x1, d1 = x1,
// d2 = x2 - x1 and the weights {g1, g2, g0 + g2, g0} give outputs 4u .. 4u + 3 from five products P1..P5 (p = 0..4):
//     P1 = d0 g1 -> 0    P2 = d1 g1 -> 0, 2    P3 = d0 g2 -> 1    P4 = d1 (g0 + g2) -> 1, 3    P5 = d2 g0 -> 3
// f22_view / f22_wt / f22_o0 / f22_o1 (-1: none) of product p; f22_cw(wt, k): coefficient of tap k in weight wt.
__host__ __device__ constexpr int f22_view(int p) { return p == 4 ? 2 : (p & 1); }
__host__ __device__ constexpr int f22_wt(int p) { return p < 2 ? 0 : p - 1; }
__host__ __device__ constexpr int f22_o0(int p) { return p < 2 ? 0 : (p < 4 ? 1 : 3); }
__host__ __device__ constexpr int f22_o1(int p) { return p == 1 ? 2 : (p == 3 ? 3 : -1); }
__host__ __device__ constexpr int f22_cw(int wt, int k) { return wt == 0 ? (k == 1) : wt == 1 ? (k == 2) : wt == 2 ? (k != 1) : (k == 0); }
// One element of the transformed weights, shared by the host packers (engine_weights.hip convt_s2_f22_weights / convt_s1_wino_weights) and the
// device repack (train_down.hip): k = the nine taps W[ci][co][.][.] of one (ci, co) pair; fp64 in this order, rounded once.
//   F(2, 2), stride-2 ConvT: U[4 wr + wc] = sum_{kh, kw} f22_cw(wr, kh) f22_cw(wc, kw) k[kh][kw]
__host__ __device__ inline float f22_u_elem(const float* k, int wr, int wc) {
#pragma clang fp contract(off)
    double s = 0;
    for (int kh = 0; kh < 3; ++kh)
        for (int kw = 0; kw < 3; ++kw) s += (double)(f22_cw(wr, kh) * f22_cw(wc, kw)) * (double)k[kh * 3 + kw];
    return (float)s;
}
//   Winograd F(2x2, 3x3), stride-1 ConvT: U[4 a + b] = (G g G^T)[a][b], g[u][v] = k[2 - u][2 - v], G = wino_g
__host__ __device__ constexpr double wino_g(int a, int u) { return a == 0 ? (u == 0 ? 1.0 : 0.0) : a == 1 ? 0.5 : a == 2 ? (u == 1 ? -0.5 : 0.5) : (u == 2 ? 1.0 : 0.0); }
__host__ __device__ inline float wino_u_elem(const float* k, int a, int b) {
#pragma clang fp contract(off)
    double Gg[3];
    for (int v = 0; v < 3; ++v) {
        double s = 0;
        for (int u = 0; u < 3; ++u) s += wino_g(a, u) * (double)k[(2 - u) * 3 + (2 - v)];
        Gg[v] = s;
    }
    double s = 0;
    for (int v = 0; v < 3; ++v) s += Gg[v] * wino_g(b, v);
    return (float)s;
}

struct DecBArgs {
    const float* y2;
    const float* w3; const float* b3;   // F(2, 2) weights packed [16 U][2 channel halves][4 chunks][64][4] (engine_weights.hip), bias [32]
    const float* w4; float b4;          // [9 taps][32 ch], scalar bias
    int rows;             // decoder rows (images) in this launch
    RowMask live;
    int m0;               // index of row 0 inside the [group][row] batch
    int rows_per_group;
    GroupMap gm;
    int reward0;          // groups with pidx == 0: 1 = reward log-likelihood, 0 = Bernoulli entropy sum (others: entropy)
    int store0;           // groups with pidx == 0 store their image at slot t*S + sample
    float* val;           // [batch] per-image pixel sum (entropy sum, or log-likelihood sum)
    int parts;            // 1 = one workgroup per image; 4 = four (small launches): quarter sums go to valq [batch][4]
    float* valq;
    float* po;            // [slots][rows_per_group][4096] stored images
    int reward_intent;    // 0 = the shipped port's NCHW-broadcast reward target, 1 = the upstream-intent variant (reward_term below)
    const void* w3b3 = nullptr;      // options mfma_bf16x3 / mfma_f16x2: ConvT3's weights as 16-bit planes [4 ks][9 taps][planes][64 lanes][8] (bf16x3.hip, k_dec_b_b3)
    int split = 0;                   // 1 = three bf16 planes, 2 = two fp16 planes
    float w3s = 1.0f, w3s_inv = 1.0f;      // fp16 split: the power of two the packed weights were scaled by, and its inverse
};
// fused encoder trunk: o [rows][64][64] -> conv1..conv4 (+ReLU) -> out [rows][576] in NHWC (p*64 + c) order
struct EncArgs {
    const float* o; float* out;
    const float* w1; const float* b1;   // conv1 [9 taps][32], [32]
    const float* w2; const float* b2;   // packed [9][1][4][64][4]
    const float* w3; const float* b3;   // packed [9][2][4][64][4]
    const float* w4; const float* b4;   // packed [9][4][4][64][4] (16x16x4 form)
    int rows;
    RowMask live;
};
void launch_enc_trunk(const EncArgs& a, hipStream_t st);
void launch_fc4(const GemmArgs& a, hipStream_t st);      // Linear(256,16384)+ReLU+Dropout with the batch tile staged in LDS
void launch_fc4_b3(const GemmArgs& a, hipStream_t st);   // the same on the bf16 pipe, operands split in three (opt-in experiment, bf16x3.hip)
float pack_dense_split(int mode, const float* W, const int* row_perm, int out, int in, uint16_t* dst);      // mode 1 = bf16 x 3, 2 = fp16 x 2; -> weight scale
void launch_dec_a_b3(const DecAArgs& a, hipStream_t st);  // k_dec_a's two layers on the bf16 pipe, every operand through LDS (opt-in experiment)
float pack_conv_split(int mode, const float* W_cicokk, int Cin, int Cout, uint16_t* dst);
void launch_dec_b_b3(const DecBArgs& a, hipStream_t st);  // k_dec_b4's layers with ConvT3 on the bf16 pipe (opt-in experiment)
float pack_convt3_split(int mode, const float* W_cicokk, uint16_t* dst);      // -> the weight scale (1 for the bf16 split)
int init_bf16x3_kernels();
void launch_dec_a(const DecAArgs& a, hipStream_t st);
void launch_dec_b(const DecBArgs& a, hipStream_t st);
// both stages in one persistent launch (k_dec_ab: parts 1 only): a.y2 = b.y2 is [grid][32 x 32 x 64], one slot per workgroup
struct DecABArgs { DecAArgs a; DecBArgs b; };
int dec_ab_grid(int rows, int cap);      // workgroups of a launch of `rows` images: min(512, rows), capped at `cap` when cap > 0
void launch_dec_ab(const DecABArgs& a, int grid_cap, hipStream_t st);

int launch_dense(int MT, int NT, const GemmArgs& a, hipStream_t st);   // 0 = launched, 1 = unsupported tile shape

struct TransPostArgs {
    const float* tr;       // [2S][R][32] (mean 0..9, logvar 10..19); group order T1_0..T1_{S-1}, T2_0..T2_{S-1}
    const float* x;        // [R][16] current [pi(4) | s0(10) | 0 0]
    const float* eps_inj;  // nullable [3S][R][10]: T1_i, T2_j, D2B_j
    const float* given_ps1;// nullable [R][10]: trajectory mode, D1 input
    float* dec_in;         // [3S][R][16]: D1_i, D2A_j, D2B_j
    float* next_x;         // nullable [R][16]
    float* ps1_last;       // nullable [R][10]
    float* ps1_mean_last;  // nullable [R][10]
    int S, R, mean_mode, carry_mean;
    uint32_t k0, k1, stage, row_offset;
    int pi_dim;            // x rows are [pi (pi_dim) | s (10) | zeros]
    const int32_t* ids; int ids_div;            // optional row identities (GroupMap)
};
void launch_trans_post(const TransPostArgs& a, hipStream_t st);

struct TermsArgs {
    const float* val;      // [D][3S][R] decoder per-image pixel sums (D1_i reward log-lik, D2A_j / D2B_j entropy)
    const float* valq;     // nullable [D][3S][R][4]: the same as quarter sums (k_dec_b4 with four workgroups per image): val = (q0 + q1) + (q2 + q3)
    const float* tr;       // [D][2S][R][32]
    const float* enc;      // [D][S][R][32]
    int D, S, R;
    float reward_div;      // term0 per image = pixel sum / reward_div * 10 (mean over the counted pixels * 10, torchmodel.py:212: 4096, or the 192 bar
                           // pixels of the upstream-intent target); 0 = the sum form of the generic geometries
    float* G;              // [R] summed over stages
    float* terms;          // [3][R] summed over stages
    float* t2parts;        // nullable [2][R]: term2_1, term2_2 (last stage; diagnostics)
};
void launch_terms(const TermsArgs& a, hipStream_t st);
int init_small_kernels();       // per-device kernel attributes (dynamic LDS above 64 KiB); 0 = ok
int init_decoder_kernels();

// ---- device-resident MCTS tree (mcts.hip) --------------------------------------------------------
struct MctsTree {
    float* W; float* N; float* Qpi;   // [E][cap][A] edge statistics of mcts.py Node (W = -sum G, N visits, Qpi habit prior)
    int32_t* child;                   // [E][cap][A] node index of each child, -1 = not expanded
    float* S;                         // [E][cap][s_dim] latent state of every node
    int E, cap, A, s_dim;
};
__device__ __forceinline__ int argmax_nan_first(const float* v, int n) {          // torch.argmax: NaN is the maximum, first index wins
    int best = 0;
    for (int i = 1; i < n; ++i) {
        const bool nb = v[best] != v[best], ni = v[i] != v[i];
        if (nb) continue;
        if (ni || v[i] > v[best]) best = i;
    }
    return best;
}
void launch_mcts_select(const MctsTree& t, const uint8_t* active, float C, int use_prior, int max_depth, int32_t* path_nodes,
                        int32_t* path_act, int32_t* path_len, int32_t* leaf, float* leaf_s, float* leaf_s_rep, hipStream_t st);
void launch_mcts_expand(const MctsTree& t, int32_t* n_nodes, const int32_t* nodes, const uint8_t* mask, const float* G,
                        const float* ps_next, hipStream_t st);
void launch_mcts_backprop(const MctsTree& t, const int32_t* path_nodes, const int32_t* path_act, const int32_t* path_len,
                          const int32_t* leaf, const uint8_t* active, const float* sims, int R, const float* q0, int max_depth,
                          float* g_out, uint8_t* active_out, hipStream_t st);
void launch_mcts_stop(const MctsTree& t, uint8_t* active, int32_t* stop_at, int repeat, float threshold, int32_t* n_active, hipStream_t st);
struct MctsStepArgs {
    // back-propagation of the previous iteration (prev_path_len == nullptr: none); path_nodes / leaf still hold that iteration's selection
    const int32_t* prev_path_act; const int32_t* prev_path_len; const float* sims; int n_sims; const float* q0; float* prev_g_out; uint8_t* prev_active_out;
    // early stop of this iteration
    uint8_t* active; int32_t* stop_at; int repeat; float threshold; int32_t* n_active;
    // selection
    float C; int use_prior, max_depth;
    int32_t *path_nodes, *path_act, *path_len, *leaf; float *leaf_s, *leaf_s_rep;
    // expansion bookkeeping of the previous iteration's leaf (exp_n_nodes == nullptr: done by the caller with efe_mcts_expand)
    int32_t* exp_n_nodes = nullptr; const float* exp_G = nullptr; const float* exp_ps_next = nullptr;
};
void launch_mcts_step(const MctsTree& t, const MctsStepArgs& a, hipStream_t st);

// ---- fused small-MLP kernels (fused.hip) ---------------------------------------------------------------------
// weights packed for v_mfma_f32_16x16x4_f32: [16-feature tile][16-channel chunk][64 lanes][4], biases padded to the tile count
struct MlpW { const float4* w[4]; const float* b[4]; };
// the dense heads next to the conv stacks, one launch each (fused.hip k_head):
//   decoder head po_net.0/.3/.6 (torchmodel.py:107-115): s[16] -> 256 -> 256 -> 256, ReLU + MC-dropout each          -> Y [M][256]
//   encoder head qs_net.9/.12/.15/.18 (torchmodel.py:94-103): flat -> 256 -> 256 -> 256 (same) -> 20 (linear)       -> Y [M][32]
struct HeadArgs {
    MlpW W;                // packed for the 16x16x4 form (pack_linear16)
    int kc0;               // 16-channel chunks of the first layer's input: X rows are 16 * kc0 floats
    int nl;                // 3: Y = the third hidden layer [M][256];  4: + a linear layer of out_tiles 16-feature tiles, Y [M][16 * out_tiles]
    int out_tiles;
    uint32_t tag0;         // noise tag of the first layer (layer i uses tag0 + i)
    const float* X; float* Y;
    int M;
    uint32_t k0, k1;
    GroupMap gm; int rows_per_group; uint32_t row_offset; int m0;
};
void launch_head(const HeadArgs& a, hipStream_t st);

struct TransFusedArgs {
    MlpW W;                // ps_net.0 / .3 / .6 / .9
    const float* X;        // [rows][16] = [pi | s0 | 0 0]
    float* tr;             // [M][32]: mean 0..9, logvar 10..19
    int M, x_mod;          // x_mod > 0: input row = m % x_mod (every MC group reads the same rows)
    uint32_t k0, k1;
    GroupMap gm; int rows_per_group; uint32_t row_offset; int m0;
};
void launch_trans_fused(const TransFusedArgs& a, hipStream_t st);
struct SimChainArgs {
    MlpW W, H;             // transition net, habit net (qpi_net.0 / .2 / .4)
    const float* s0;       // [E][10] starting states
    int E, T, use_means;
    uint32_t k0, k1, stage, row_offset;
    const float* eps_inj;  // nullable [T][E][10]
    const float* u_inj;    // nullable [T][E]
    float *s0_traj, *ps1_traj, *mean_traj, *lv_traj;   // [E][T][10]
    float* pi0;            // [E][T][pi_dim] one-hot
    float* Qpi0;           // nullable [E][pi_dim]
    float* tr;             // nullable [2][E * T][32]: the trajectory core's transition rows (given T1 | T2 of the same input)
    int pi_dim;
    const int32_t* ids;                         // optional episode identities: episode slot e is episode ids[e] of the un-compacted batch
    // optional (one-episode decisions): a group of 8 episodes on EIGHT workgroups that split the two wide transition layers; exchange buffer
    // [groups][2][16][512] floats and self-resetting counters [groups][4] ints (zero at first use), both owned by the context
    float* xch = nullptr; int* sync = nullptr;
};
constexpr int SIM_FE = 8;                        // episodes per group of the simulation chain kernel
constexpr int SIM_MAX_SPLIT_GROUPS = 2;          // launches of up to 16 episodes use the split form
void launch_sim_chain(const SimChainArgs& a, hipStream_t st);
int init_fused_kernels();

// ---- geometry-generic convolution path (generic.hip) ---------------------------------------------
struct ConvGArgs {
    const float* in; float* out;      // NHWC activations
    const float* Wp; const float* bias; const float* zeros;     // packed [tap][32-feature tile][8-channel chunk][64 lanes][4]
    int n_img, Hin, Win, Cin;         // Cin padded to a multiple of 8
    int Hout, Wout, Cout, mtiles;
    int mode;                         // 0 Conv2d(k3,s2,p0)   1 ConvTranspose2d(k3,s1,p1)   2 ConvTranspose2d(k3,s2,p1,op1), sub-pixel form
    int relu;
    int ldo;                          // floats per output pixel
    RowMask live;                     // LDS-tiled ConvT kernels only (the decoder's layers)
};
void launch_conv_g(const ConvGArgs& a, hipStream_t st);
bool convt_p_ok(const ConvGArgs& a);                            // generic_dec.hip: the LDS-tiled ConvTranspose kernel takes this layer
void launch_convt_p(const ConvGArgs& a, hipStream_t st);
// ConvT(64,64,s1) + ReLU + ConvT(64,64,s2) + ReLU in one kernel, layer 1's output kept in LDS (generic_dec.hip: k_convt_12)
struct ConvT12Args {
    const float* in; float* out;        // [n][Hin * Win][64] -> [n][4 Hin * Win][64], NHWC
    const float* W1p; const float* b1;  // layer 1 as ConvGArgs::Wp / bias (packed [9][2][8][64][4])
    const float* W2p; const float* b2;  // layer 2
    int n_img, Hin, Win;
    RowMask live;
};
int launch_convt_12(const ConvT12Args& a, hipStream_t st);      // non-zero: outside the kernel's limits (launch the layers one by one)
// fused last two decoder layers of the generic path (generic_dec.hip): y2 [rows][Hin * Win][64] NHWC -> per-image sums (+ stored images)
struct DecBGArgs {
    const float* y2;
    const float* w3; const float* b3;   // packed [9][1][8][64][4], bias [32]
    const float* w4; float b4[4];       // [9 taps][32 ci][4 c], bias
    int rows, m0, rows_per_group, Hin, Win, C;
    int TH, RPa; unsigned magicWin;     // set by launch_dec_bg: input rows per strip, ring slots of the LDS strip, ceil(2^32 / Win)
    GroupMap gm;
    int reward0, store0, reward_intent;
    RowMask live;
    float* val;                         // [batch] per-image sums
    float* po;                          // [slots][rows_per_group][Hout * Wout][4] stored images (NHWC, channels padded to 4)
};
// LDS-tiled encoder Conv2d(k3, s2, p0) + ReLU of the generic path, layers 1 and 2 (generic_enc.hip)
struct ConvEArgs {
    const float* in;                    // layer 1: NHWC4 image [n][Hin * Win][4]; layer 2: [n][Hin * Win][32]
    float* out;                         // [n][Hout * Wout][32]
    const float* Wp; const float* bias; // layer 2: packed [9][1][4][64][4]; layer 1: [9 taps][64 lanes][2] = W[co][h][tap], W[co][2 + h][tap]
    int n_img, Hin, Win, Hout, Wout;
    int TY; unsigned magicWin, magicWout;       // set by launch_conv_e
    RowMask live;
};
int launch_conv_e(ConvEArgs a, int layer, hipStream_t st);     // non-zero: outside the kernel's limits (use k_conv_g)
// the two layers in one kernel, conv1's output kept in LDS (generic_enc.hip: k_conv_e12)
struct ConvE12Args {
    const float* in;                    // NHWC4 image [n][H0 * W0][4]
    float* out;                         // [n][H2 * W2][32]
    const float* W1p; const float* b1;  // layer 1 as ConvEArgs::Wp / bias of layer 1
    const float* W2p; const float* b2;  // layer 2 as ConvEArgs::Wp / bias of layer 2
    int n_img, H0, W0, H1, W1, H2, W2;
    int TY; unsigned magicW1, magicW2;          // set by launch_conv_e12
    RowMask live;
};
int launch_conv_e12(ConvE12Args a, hipStream_t st);             // non-zero: outside the kernel's limits (launch the layers one by one)
int init_generic_enc_kernels();
int launch_dec_bg(DecBGArgs a, hipStream_t st);                 // non-zero: geometry outside the kernel's limits
bool dec_bg_ok(int Hin, int Win, int C);                        // the fused kernel takes this geometry (decided before scratch is sized)
int init_generic_dec_kernels();
struct FinalGArgs {
    const float* y3;                  // [rows][H*W][32]
    const float* w; float b[4];       // [9 taps][32 ci][4 c], bias
    int rows, m0, rows_per_group, H, W, C;
    GroupMap gm;
    int reward0, store0, reward_intent;
    RowMask live;
    float* val;                       // [batch] per-image sums
    float* po;                        // [slots][rows_per_group][H*W][4] stored images (NHWC, channels padded to 4)
};
int launch_final_g(const FinalGArgs& a, hipStream_t st);       // non-zero: geometry outside the kernel's limits (W <= 128, C <= 3)
int init_generic_kernels();
constexpr int GEN_IMG_LD = 4;          // floats per pixel of the generic path's stored images (NHWC, C <= 3 channels padded to 4)
void launch_to_nhwc4(const float* in, float* out, long M, int HW, int C, hipStream_t st);       // NCHW -> NHWC4
void launch_nhwc4_to_8(const float* in, float* out, long n_pix, hipStream_t st);                // NHWC4 -> NHWC8 (k_conv_g's first layer contracts 8 input channels)
void launch_to_nchw(const float* in, float* out, long M, int HW, int C, hipStream_t st);
void launch_check_reward_g(const float* o, float* out, int M, int C, int H, int W, int intent, hipStream_t st);

// forward free energy (loss.hip): per-row tails of compute_loss_top / _mid / _down.  Row r of every [M]/[M][k] array is row r of the call.
constexpr int S_DIM_FE = 10;
struct FeArgs {
    int M, A;                                           // rows of the call, pi_dim
    // top: Qpi, log_Qpi [M][A] (habit head), log_Ppi [M][A]; q == nullptr: no top part
    const float* q; const float* logq; const float* log_Ppi;
    float* kl_pi_anal; float* kl_pi; float* F_top;
    // omega: 0 = omega_in [M], 1 = omega_scalar, 2 = compute_omega(kl_pi, oa_a, oa_b, oa_c, oa_d) (k_fe_top_mid only); omega_out [M] nullable
    int omega_mode; const float* omega_in; float omega_scalar; float oa_a, oa_b, oa_c, oa_d;
    float* omega_out;
    // posterior q(s1) and prior p(s1) means / logvars, row strides q1_ld / p1_ld; q1_mean == nullptr in k_fe_top_mid: no mid part
    const float* q1_mean; const float* q1_lv; int q1_ld;
    const float* p1_mean; const float* p1_lv; int p1_ld;
    float* kl_mid_anal; float* kl_mid; float* F_mid;
    // down: o1 NCHW [M][C*HW]; the image block handed to launch_fe_down is NCHW, or NHWC4 (generic store) when nhwc4
    const float* o1; int C, HW, nhwc4;
    float gamma, beta_s, beta_o;
    float* F_down; float* nlogpo1; float* kl_s; float* kl_s_anal; float* kl_naive; float* kl_naive_anal;
};
void launch_fe_top_mid(const FeArgs& a, hipStream_t st);
void launch_fe_down(const FeArgs& a, const float* po, int m0, int rows, hipStream_t st);     // rows [m0, m0 + rows); po = their images
// the training step's tails (loss.hip): omega_out[r] = row omega of kl_pi[r] (FeArgs: M, kl_pi, the omega fields, omega_out), and the
// step's statistics: means[q] = mean of x[q] [M] for q < 7 (kl_pi, omega, F_mid, F_down, nlogpo1, kl_s, kl_naive), means[7] = std of x[1]
constexpr int STEP_MEANS = 8;          // = EFE_STEP_MEANS (include/efe_engine.h)
struct StepMeansArgs { const float* x[STEP_MEANS - 1]; float* means; int M; };
void launch_step_omega(const FeArgs& a, hipStream_t st);
void launch_step_means(const StepMeansArgs& a, hipStream_t st);
// the epoch report (eval.hip): one row of EVAL_STATS floats from the per-row arrays of an evaluation batch; a group whose first pointer
// is null is absent and its fields are written as NaN (layout and groups: include/efe_engine.h efe_eval_stats)
constexpr int EVAL_STATS = 98;         // = EFE_EVAL_STATS
constexpr int EVAL_MAX_ROWS = 8192;    // = EFE_EVAL_MAX_ROWS: one column of floats in LDS (32 KiB), 4 M^4 < 2^63
constexpr int EVAL_FACTORS = 6;        // columns of S_real
struct EvalArgs {
    const float* row[7];               // FE: F_top, F_mid, F_down, nlogpo1, kl_s, kl_naive, kl_pi [M]
    const float* kl_s_anal; const float* kl_naive_anal; const float* kl_pi_anal;      // [M][10], [M][10], [M][A]
    const float* qs1;                  // TC: [M][10]
    const float* s0; const float* S_real;      // RHO: [M][10], [M][EVAL_FACTORS]
    const float* o1_r; const float* po1_r;     // R: [Mr][4096] NCHW, C = 1
    int M, Mr, A;
    float* out;                        // [EVAL_STATS]
};
void launch_eval_stats(const EvalArgs& a, hipStream_t st);
// the mutual information of every latent with every true factor (eval.hip, efe_eval_mi): the KSG k-nearest-neighbour estimator in fp64
constexpr int EVAL_MI = 60;            // = EFE_EVAL_MI: pairs, latent-major
constexpr int EVAL_MI_MAX_K = 4;       // = EFE_EVAL_MI_MAX_NEIGHBORS
constexpr int EVAL_MI_POINTS = 256;    // points of one workgroup of the pair sweep = its j tile = its threads
constexpr int EVAL_MI_SLICES = EVAL_MAX_ROWS / EVAL_MI_POINTS;      // workgroups of one pair at the row cap
constexpr size_t EVAL_MI_WS = 32 + (size_t)EVAL_MI * EVAL_MI_SLICES * 2;      // doubles: column statistics, then the per-slice partial sums
constexpr int EVAL_MI_PSI = EVAL_MAX_ROWS + 2;      // entries of the digamma table: the integers 0 .. 8193
struct EvalMiArgs {
    const float* s0; const float* S_real;      // [M][10], [M][EVAL_FACTORS]
    const double* noise;               // [EVAL_MI][2][M], or null: drawn under TAG_MI from (k0, k1), row j, stream_id(pair, which), stage
    int M, k;
    uint32_t k0, k1, stage;
    double* ws;                        // [EVAL_MI_WS]
    const double* psi;                 // [EVAL_MI_PSI]: digamma at the integers (eval_mi_psi_table)
    float* out;                        // [EVAL_MI]
    int32_t* counts;                   // null, or [EVAL_MI][2][M]
};
void launch_eval_mi(const EvalMiArgs& a, hipStream_t st);
void eval_mi_psi_table(double* t);     // host: fills t[EVAL_MI_PSI]

// ---- training of the small MLPs (train.hip): backward + Adam over a layer table -----------------------------------
// A trainable part is a chain of Linear layers described by a DEVICE-RESIDENT table (built at efe_commit_weights): widths, the ReLU flag
// of each layer's output, the Philox tag of the MC-dropout mask behind it (0 = no dropout: the habit net; the transition net's hidden
// layers carry TAG_MID + layer, drawn in k_mid_grad's forward pass), the offsets of the layer's weight / bias inside the flat parameter
// vector (the reference's parameters() order, row-major) and the packed forward copies k_adam refreshes.
constexpr int TRAIN_MAX_LAYERS = 4;      // layers of a table
constexpr int TRAIN_MAX_WIDTH = 128;     // widest activation k_top_grad keeps in LDS
constexpr int TRAIN_MAX_SLABS = 64;      // workgroups (= partial-gradient slabs) of one k_top_grad launch
constexpr int TRAIN_MAX_A = 8;           // widest categorical head
struct TrainLayer {
    int in, out, relu, drop_tag;
    int w_off, b_off;                    // offsets in the flat parameter vector
    int kc32, kc16;                      // K chunks of the two packed forms (upload_packed: 8 channels, pack_linear16: 16 channels)
    float *Wp32, *b32, *Wp16, *b16;      // packed copies read by the forward paths
};
struct TrainNet { int nl, P; float* master; TrainLayer L[TRAIN_MAX_LAYERS]; };
__host__ __device__ inline int train_slabs(int M) { const int t = (M + 15) / 16; return t < TRAIN_MAX_SLABS ? t : TRAIN_MAX_SLABS; }
struct TrainKey { uint32_t k0, k1, row0, stream, stage; };     // Philox fields of a training call: key, global row of row 0, stream_id(pass, sample), stage
struct TopGradArgs {
    const TrainNet* net;                 // device pointer
    const float* s; const float* log_Ppi;       // [M][in of layer 0], [M][A]
    float* kl_pi;                        // nullable [M]
    float* slabs;                        // [train_slabs(M)][P] partial gradients (slab p = workgroup p)
    int M, A;
    float inv_M;
};
void launch_top_grad(const TopGradArgs& a, hipStream_t st);
void launch_slab_sum(const float* slabs, int nslab, int P, float* grad, hipStream_t st);
struct AdamArgs {
    const TrainNet* net;                 // device pointer
    const float* g; int nslab;           // gradient = g[0][i] + g[1][i] + ... in ascending slab order (nslab = 1: a plain gradient)
    float* m; float* v;                  // exp_avg, exp_avg_sq [P]
    float omb1, b2, omb2;                // 1 - beta1, beta2, 1 - beta2
    float bc2_sqrt, step_size, eps;      // sqrt(1 - beta2^t), lr / (1 - beta1^t)
};
void launch_adam(const AdamArgs& a, int P, hipStream_t st);
// torch.optim.Adam, default flags (no amsgrad, no weight decay, not maximize), one element, in this order:
//   m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  denom = sqrt(v) / sqrt(1 - b2^t) + eps;  w = w + (-(lr / (1 - b1^t)) m) / denom
// Contraction off, division and square root correctly rounded; the bias corrections come from the host (double, rounded once).  Shared by
// k_adam (train.hip) and k_adam_down (train_down.hip).
__device__ __forceinline__ void adam_update(float g, float& m, float& v, float& wv, float omb1, float b2, float omb2, float bc2_sqrt, float step_size,
                                            float eps) {
#pragma clang fp contract(off)
    m = m + omb1 * (g - m);
    v = b2 * v + (omb2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), bc2_sqrt) + eps;
    wv = wv + __fdiv_rn(-step_size * m, denom);        // addcdiv_(m, denom, value = -step_size): (value * m) / denom
}
// the transition net ModelMid.ps_net (k_mid_grad): hidden layers up to TRAIN_MID_WIDTH wide, each ReLU + MC-dropout; one partial-gradient
// slab is 2.17 MB (P = 543 252 at pi_dim 4), so the workgroup count has a cap of its own
constexpr int TRAIN_MID_WIDTH = 512;     // widest hidden activation k_mid_grad keeps in LDS
constexpr int TRAIN_MID_IN = 16;         // widest input (pi_dim + s_dim, padded to one 16-channel chunk)
constexpr int TRAIN_MID_OUT = 32;        // widest output (2 s_dim, padded to two 16-feature tiles)
constexpr int TRAIN_MID_SLABS = 8;       // workgroups (= slabs) of one k_mid_grad launch: 17 MB of scratch at the cap
__host__ __device__ inline int train_mid_slabs(int M) { const int t = (M + 15) / 16; return t < TRAIN_MID_SLABS ? t : TRAIN_MID_SLABS; }
struct MidGradArgs {
    const TrainNet* net;                 // device pointer
    const float* s0; const float* pi0;   // [M][s_dim], [M][A]: the input row is [pi0 | s0] (torchmodel.py:59)
    const float* q1_mean; const float* q1_lv;   // [M][s_dim] posterior q(s1)
    int omega_mode; const float* omega_in; float omega_scalar;      // 0 = omega_in [M], 1 = omega_scalar
    float* p1_mean; float* p1_lv; float* F_mid; // outputs [M][s_dim], [M][s_dim], [M] (the host hands scratch for those the caller declines)
    float* slabs;                        // [train_mid_slabs(M)][P]
    int M, A, S;
    float inv_M;
    TrainKey key;
};
void launch_mid_grad(const MidGradArgs& a, hipStream_t st);
int init_train_kernels();

// ---- backward of the decoder's ConvTranspose2d tail po_net[12:] at 1 x 64 x 64 (train_dec.hip) -----------------------------
// The parameters as one flat vector in parameters() order (13.weight, 13.bias, 15.weight, 15.bias, 17.weight, 17.bias, 19.weight, 19.bias),
// each tensor row-major in the reference's shape ([Cin][Cout][3][3]): the layout of the raw device copy and of the gradient.
constexpr int DT_W1 = 0, DT_B1 = DT_W1 + 64 * 64 * 9, DT_W2 = DT_B1 + 64, DT_B2 = DT_W2 + 64 * 64 * 9, DT_W3 = DT_B2 + 64,
              DT_B3 = DT_W3 + 64 * 32 * 9, DT_W4 = DT_B3 + 32, DT_B4 = DT_W4 + 32 * 9, DEC_TAIL_P = DT_B4 + 1;      // 92 609
constexpr int DEC_TAIL_SLABS = 32;       // partial-gradient slabs: row m adds to slab m mod G, G = dec_tail_slabs(M)
constexpr int DEC_TAIL_ROWS = 64;        // rows per pass (a multiple of DEC_TAIL_SLABS): bounds the stored activations and gradients
constexpr size_t DEC_TAIL_Y1 = 64 * 256, DEC_TAIL_Y2 = 64 * 1024, DEC_TAIL_Y3 = 32 * 4096;      // floats per row
__host__ __device__ inline int dec_tail_slabs(int M) { return M < DEC_TAIL_SLABS ? M : DEC_TAIL_SLABS; }
struct DecTailArgs {                     // one row group: every pointer is the group's first row
    const float* w;                      // raw parameters [DEC_TAIL_P]
    const float* h4; const float* o1;    // [rows][64][16][16], [rows][4096]
    float *y1, *y2, *y3, *po;            // stored forward
    float* nlogpo1;                      // [rows]
    float *g4, *g3, *g2, *g1;            // dL / da_l
    float* dh4;                          // nullable [rows][64][16][16]
    float* slabs;                        // [G][DEC_TAIL_P]; first != 0: written, else added to
    int rows, G, first;
    float scale;
};
void launch_dec_tail_group(const DecTailArgs& a, hipStream_t st);

// ---- the same backward at every admitted geometry (train_dec_g.hip): B = the decoder's base grid, C colour channels, S3 = layer 3's stride --
// The flat vector keeps DT_W1 .. DT_B3; layer 4 is [32][C][3][3] then [C]: P = 92 320 + 289 C.
struct DecTailGeo {
    int B, C, S3;
    __host__ __device__ int R() const { return S3 * 2 * B; }                       // the resolution
    __host__ __device__ int w4() const { return DT_W4; }
    __host__ __device__ int b4() const { return DT_W4 + 288 * C; }
    __host__ __device__ int P() const { return DT_W4 + 289 * C; }
    size_t y1() const { return (size_t)64 * B * B; }                               // floats per row
    size_t y2() const { return (size_t)64 * 4 * B * B; }
    size_t y3() const { return (size_t)32 * R() * R(); }
    size_t img() const { return (size_t)C * R() * R(); }
    int rows_per_pass() const { return B <= 16 ? 64 : 32; }                        // a multiple of DEC_TAIL_SLABS, a function of the geometry alone
};
struct DecTailGArgs {                    // one row group: every pointer is the group's first row
    DecTailGeo geo;
    const float* w;                      // raw parameters [P]
    const float* h4; const float* o1;    // [rows][64][B][B], [rows][C][R][R]
    float *y1, *y2, *y3, *po;            // stored forward
    float* nlogpo1;                      // [rows]
    float *g4, *g3, *g2, *g1;            // dL / da_l
    float* dh4;                          // nullable [rows][64][B][B]
    float* slabs;                        // [G][P]; first != 0: written, else added to
    int rows, G, first;
    float scale;
};
void launch_dec_tail_g_group(const DecTailGArgs& a, hipStream_t st);

// ---- backward of the decoder's dense head po_net[0:12] at 1 x 64 x 64 (train_dec_head.hip) ---------------------------------
// The whole po_net as one flat vector in parameters() order: 0.weight [256][10], 0.bias, 3.weight [256][256], 3.bias, 6.weight, 6.bias,
// 9.weight [16384][256], 9.bias, then the tail's DEC_TAIL_P (DT_* offsets behind DEC_HEAD_P): the raw device copy and the gradient.
constexpr int DH_W0 = 0, DH_B0 = DH_W0 + 256 * 10, DH_W1 = DH_B0 + 256, DH_B1 = DH_W1 + 256 * 256, DH_W2 = DH_B1 + 256, DH_B2 = DH_W2 + 256 * 256,
              DEC_HEAD_SMALL_P = DH_B2 + 256,                                     // 134 400: one partial-gradient slab of layers 0..2
              DH_W3 = DEC_HEAD_SMALL_P, DH_B3 = DH_W3 + 16384 * 256, DEC_HEAD_P = DH_B3 + 16384, DEC_P = DEC_HEAD_P + DEC_TAIL_P;      // 4 345 088, 4 437 697
constexpr int DEC_HEAD_SLABS = 4;        // slabs of layers 0..2: 16-row tile t adds to slab t mod G, G = dec_head_slabs(M) (four tiles per row group)
constexpr int DEC_HEAD_SEGS = 64;        // K segments (256 features each) of d_h3 = g4 W4
__host__ __device__ inline int dec_head_slabs(int M) { const int t = (M + 15) / 16; return t < DEC_HEAD_SLABS ? t : DEC_HEAD_SLABS; }
struct DecHeadArgs {                     // one row group (at most DEC_TAIL_ROWS rows): every row pointer is the group's first row
    const float* w;                      // raw parameters [DEC_P]
    const float* s;                      // [rows][10]
    float *h1, *h2, *h3, *h4;            // stored forward, after the mask: [rows][256] x 3, [rows][16384] (reference order c 256 + p)
    float* g4;                           // in: d_h4 [rows][16384] of the tail; gated in place to dL / da of layer 3
    float* part;                         // [DEC_HEAD_SEGS][rows][256] partial sums of g4 W4
    float* ds;                           // nullable [rows][10]
    float* grad;                         // the caller's gradient [DEC_P]: 9.weight / 9.bias are written (first) or added to in place
    float* slabs;                        // [G][DEC_HEAD_SMALL_P]; first != 0: written, else added to
    int rows, first;
    TrainKey key;                        // row0 = the global row of the group's row 0
};
void launch_dec_head_fwd(const DecHeadArgs& a, hipStream_t st);       // s -> h1 .. h4
void launch_dec_head_bwd(const DecHeadArgs& a, hipStream_t st);       // d_h4 -> the head's gradients and d_s
void launch_dec_head_fwd_small(const DecHeadArgs& a, hipStream_t st); // layers 0..2 alone (k_dech_fwd): s -> h1 .. h3, at any geometry
void launch_dec_head_gate(const float* h4, float* g, size_t n, hipStream_t st);      // k_dech_gate over n elements (a multiple of 4)

// ---- the same head at every admitted geometry (train_dec_head_g.hip): F = 64 B^2 features of po_net.9, from the context ---------------
// The flat vector keeps DH_W0 .. DH_B2; 9.weight is [F][256] at DH_W3, 9.bias [F] behind it, then the tail's DecTailGeo::P() floats.
struct DecHeadGeo {
    int B;
    __host__ __device__ int BB() const { return B * B; }                           // pixels of the base grid = features per channel
    __host__ __device__ int F() const { return 64 * B * B; }                       // 5 184 .. 65 536, a multiple of 64
    __host__ __device__ size_t b3() const { return (size_t)DH_W3 + (size_t)F() * 256; }
    __host__ __device__ size_t P() const { return b3() + (size_t)F(); }            // 134 400 + 257 F
    __host__ __device__ int segs() const { return (F() + 255) / 256; }             // K segments of d_h3 = g4 W3; the last holds 64 features at odd B
};
struct DecHeadGArgs {                    // one row group (DecTailGeo::rows_per_pass() rows at most): every row pointer is the group's first row
    DecHeadGeo geo;
    const float* w;                      // raw parameters [geo.P() + the tail's]
    const float* s;                      // [rows][10]
    float *h1, *h2, *h3, *h4;            // stored forward, after the mask: [rows][256] x 3, [rows][F] (reference order c B^2 + p)
    float* g4;                           // in: d_h4 [rows][F] of the tail; gated in place to dL / da of layer 3
    float* part;                         // [geo.segs()][rows][256] partial sums of g4 W3; k_dechg_join leaves g_2 [rows][256] in plane 0
    float* ds;                           // nullable [rows][10]
    float* grad;                         // the caller's gradient: 9.weight / 9.bias are written (first) or added to in place
    float* slabs;                        // [G][DEC_HEAD_SMALL_P]; a tile writes its slab if it is the slab's first, else adds to it
    int rows, first;                     // first: the call's first row group
    int tile0;                           // global index of the group's first 16-row tile: tile t of the call goes to slab t mod DEC_HEAD_SLABS
    TrainKey key;                        // row0 = the global row of the group's row 0
};
void launch_dec_head_g_fwd(const DecHeadGArgs& a, hipStream_t st);    // s -> h1 .. h4
void launch_dec_head_g_bwd(const DecHeadGArgs& a, hipStream_t st);    // d_h4 -> the head's gradients and d_s

// ---- training forward and backward of the encoder qs_net at 1 x 64 x 64 (train_enc.hip) -----------------------------------------
// The whole qs_net as one flat vector in parameters() order: 0.weight [32][1][3][3], 0.bias, 2.weight [32][32][3][3], 2.bias, 4.weight
// [64][32][3][3], 4.bias, 6.weight [64][64][3][3], 6.bias, 9.weight [256][576], 9.bias, 12.weight [256][256], 12.bias, 15.weight, 15.bias,
// 18.weight [20][256], 18.bias: the raw device copy and the gradient.  The convolutions come first (ENC_CONV_P), the dense head behind.
constexpr int EQ_W1 = 0, EQ_B1 = EQ_W1 + 32 * 9, EQ_W2 = EQ_B1 + 32, EQ_B2 = EQ_W2 + 32 * 32 * 9, EQ_W3 = EQ_B2 + 32, EQ_B3 = EQ_W3 + 64 * 32 * 9,
              EQ_W4 = EQ_B3 + 64, EQ_B4 = EQ_W4 + 64 * 64 * 9, ENC_CONV_P = EQ_B4 + 64,                                  // 64 992
              EQ_W9 = ENC_CONV_P, EQ_B9 = EQ_W9 + 256 * 576, EQ_W12 = EQ_B9 + 256, EQ_B12 = EQ_W12 + 256 * 256, EQ_W15 = EQ_B12 + 256,
              EQ_B15 = EQ_W15 + 256 * 256, EQ_W18 = EQ_B15 + 256, EQ_B18 = EQ_W18 + 20 * 256, ENC_P = EQ_B18 + 20,        // 349 428
              ENC_HEAD_P = ENC_P - ENC_CONV_P, DOWN_P = ENC_P + DEC_P;                                                   // 284 436, 4 787 125
constexpr size_t ENC_Y1 = 32 * 961, ENC_Y2 = 32 * 225, ENC_Y3 = 64 * 49, ENC_Y4 = 64 * 9;      // floats per row of the stored activations
constexpr int ENC_CONV_SLABS = 32;       // slabs of the convolutions' gradient: row m adds to slab m mod G, G = enc_conv_slabs(M)
constexpr int ENC_HEAD_SLABS = 4;        // slabs of the dense head's: 16-row tile t adds to slab t mod G, G = enc_head_slabs(M)
__host__ __device__ inline int enc_conv_slabs(int M) { return M < ENC_CONV_SLABS ? M : ENC_CONV_SLABS; }
__host__ __device__ inline int enc_head_slabs(int M) { const int t = (M + 15) / 16; return t < ENC_HEAD_SLABS ? t : ENC_HEAD_SLABS; }
struct EncTrainArgs {                    // one row group (at most DEC_TAIL_ROWS rows): every row pointer is the group's first row
    const float* w;                      // raw parameters [ENC_P]
    const float* o;                      // [rows][64][64]
    float *y1, *y2, *y3, *y4;            // stored forward: relu outputs [rows][32][31][31], [32][15][15], [64][7][7], [64][3][3] (NCHW)
    float *h1, *h2, *h3;                 // ... of the head, after the mask [rows][256]
    float *mean, *logvar;                // [rows][10]
    const float *g_mean, *g_logvar;      // backward: the upstream pair [rows][10]
    float *g4, *g3, *g2, *g1;            // dL / da of the four convolutions, shaped as y4 .. y1
    float* cslabs;                       // [GC][ENC_CONV_P]; first != 0: written, else added to
    float* hslabs;                       // [GH][ENC_HEAD_P]
    int rows, GC, first;
    TrainKey key;                        // row0 = the global row of the group's row 0
};
void launch_enc_train_fwd(const EncTrainArgs& a, hipStream_t st);     // o -> y1 .. y4, h1 .. h3, mean, logvar
void launch_enc_train_bwd(const EncTrainArgs& a, hipStream_t st);     // (g_mean, g_logvar) -> the slabs of every parameter's gradient

// ---- the same encoder at every admitted geometry (train_enc_g.hip): C input channels, resolution R, from the context ------------------
// The flat vector in parameters() order: 0.weight [32][C][3][3], 0.bias, 2.weight .. 6.bias as above, 9.weight [256][K], 9.bias, then
// 12.weight .. 18.bias (ENC_SMALL_P floats, the part whose gradient goes through the head's slabs).  P = 201 684 + 288 C + 256 K.
constexpr int ENC_SMALL_P = 2 * (256 * 256 + 256) + 20 * 256 + 20;                  // 136 724: 12.weight .. 18.bias
constexpr int EQS_W12 = 0, EQS_B12 = EQS_W12 + 256 * 256, EQS_W15 = EQS_B12 + 256, EQS_B15 = EQS_W15 + 256 * 256, EQS_W18 = EQS_B15 + 256,
              EQS_B18 = EQS_W18 + 20 * 256;                                          // offsets inside that part
struct EncGeo {
    int C, R;
    __host__ __device__ static int down(int h) { return (h - 3) / 2 + 1; }
    __host__ __device__ int H1() const { return down(R); }                          // 15 .. 63
    __host__ __device__ int H2() const { return down(H1()); }                       //  7 .. 31
    __host__ __device__ int H3() const { return down(H2()); }                       //  3 .. 15
    __host__ __device__ int H4() const { return down(H3()); }                       //  1 ..  7
    __host__ __device__ int K() const { return 64 * H4() * H4(); }                  // inputs of qs_net.9: 64 .. 3 136, a multiple of 64
    __host__ __device__ int segs() const { return (K() + 255) / 256; }              // K segments of W9 y4: 1 .. 13, the last may hold 64 inputs
    __host__ __device__ int w1() const { return 0; }
    __host__ __device__ int b1() const { return 288 * C; }
    __host__ __device__ int w2() const { return b1() + 32; }
    __host__ __device__ int b2() const { return w2() + 32 * 32 * 9; }
    __host__ __device__ int w3() const { return b2() + 32; }
    __host__ __device__ int b3() const { return w3() + 64 * 32 * 9; }
    __host__ __device__ int w4() const { return b3() + 64; }
    __host__ __device__ int b4() const { return w4() + 64 * 64 * 9; }
    __host__ __device__ int conv_P() const { return b4() + 64; }                    // 64 704 + 288 C: one slab of the convolutions' gradient
    __host__ __device__ int w9() const { return conv_P(); }
    __host__ __device__ int b9() const { return w9() + 256 * K(); }
    __host__ __device__ int small() const { return b9() + 256; }                    // 12.weight: where the ENC_SMALL_P floats begin
    __host__ __device__ int P() const { return small() + ENC_SMALL_P; }
    size_t img() const { return (size_t)C * R * R; }                                // floats per row
    size_t y1() const { return (size_t)32 * H1() * H1(); }
    size_t y2() const { return (size_t)32 * H2() * H2(); }
    size_t y3() const { return (size_t)64 * H3() * H3(); }
    size_t y4() const { return (size_t)K(); }
};
struct EncTrainGArgs {                   // one row group (DecTailGeo::rows_per_pass() rows at most): every row pointer is the group's first row
    EncGeo geo;
    const float* w;                      // raw parameters [geo.P()]
    const float* o;                      // [rows][C][R][R], the caller's NCHW image
    float *y1, *y2, *y3, *y4;            // stored forward: relu outputs [rows][32][H1][H1], [32][H2][H2], [64][H3][H3], [64][H4][H4] (NCHW)
    float *h1, *h2, *h3;                 // ... of the head, after the mask [rows][256]
    float *mean, *logvar;                // [rows][10]
    const float *g_mean, *g_logvar;      // backward: the upstream pair [rows][10]
    float *g4, *g3, *g2, *g1;            // dL / da of the four convolutions, shaped as y4 .. y1
    float* part;                         // [geo.segs()][rows][256] partial sums of W9 y4
    float* g0;                           // [rows][256] dL / da of qs_net.9
    float* grad;                         // the caller's gradient: 9.weight / 9.bias are written (first) or added to in place
    float* cslabs;                       // [GC][geo.conv_P()]; first != 0: written, else added to
    float* hslabs;                       // [GH][ENC_SMALL_P]; a tile writes its slab if it is the slab's first, else adds to it
    int rows, GC, first;                 // first: the call's first row group
    int tile0;                           // global index of the group's first 16-row tile: tile t of the call goes to slab t mod ENC_HEAD_SLABS
    TrainKey key;                        // row0 = the global row of the group's row 0
};
void launch_enc_train_g_fwd(const EncTrainGArgs& a, hipStream_t st);  // o -> y1 .. y4, h1 .. h3, mean, logvar
void launch_enc_train_g_bwd(const EncTrainGArgs& a, hipStream_t st);  // (g_mean, g_logvar) -> every parameter's gradient (slabs, 9.* in place)
// d mean(F_down) / d (qs1_mean, qs1_logvar) of one row group: the decoder's d_s through the sample plus the two KL terms of compute_loss_down
struct DownLatentArgs {
    const float *d_s, *mean, *logvar, *p1_mean, *p1_lv;      // [rows][10] each
    const float* eps_inj;                // nullable [rows][10]: else the draw of (TAG_EPS, key)
    const float* omega_in; float omega_scalar;      // omega_in nullable [rows]
    float gamma, beta_s, Mf;             // Mf = the rows of the whole call (the mean's divisor)
    float *g_mean, *g_logvar;            // [rows][10]
    int rows;
    TrainKey key;
};
void launch_down_latent(const DownLatentArgs& a, hipStream_t st);

// ---- the optimiser step of ModelDown at 1 x 64 x 64 (train_down.hip): Adam over the flat [DOWN_P] vector, then the packed forms again ------
struct DownAdamArgs {
    const float* g;                      // gradient [P], already slab-summed
    float *m, *v, *w;                    // exp_avg, exp_avg_sq, the raw master copy [P]
    int P;
    float omb1, b2, omb2, bc2_sqrt, step_size, eps;      // as AdamArgs
};
void launch_adam_down(const DownAdamArgs& a, hipStream_t st);
// One packed buffer of the forward paths as k_repack_down rebuilds it from the raw copy: the inverse of the host packer named per kind
// (engine_weights.hip).  n = owning threads: destination floats (RP_BIAS, RP_TAP32) or destination float4s (the fragment forms).
enum RepackKind {
    RP_BIAS,        // bias padded with zeros to n (upload_layer / pack_linear16), rows optionally permuted
    RP_TAP32,       // [tap][32] of a [32][9] tensor: the encoder's conv1, the decoder's final convolution
    RP_DENSE32,     // pack_linear -> upload_packed: 32x32x2 fragment order, rows / columns optionally permuted
    RP_DENSE16,     // pack_linear16: 16x16x4 fragment order, columns optionally permuted
    RP_CONV32,      // pack_conv (Conv2d): nine taps of the 32x32x2 form
    RP_CONV16,      // the encoder's conv4 in the 16x16x4 form
    RP_WINO,        // convt_s1_wino_weights as 16 taps of the 32x32x2 form
    RP_F22          // pack_u16x16x4(convt_s2_f22_weights)
};
struct RepackDesc {
    float* dst; int src;                 // the packed buffer; offset of the source tensor in the raw copy
    int kind, n, block0;                 // RepackKind; owning threads; the first workgroup of this entry (256 threads each)
    int out, in, KC, mtiles;             // the tensor's rows / columns (Cout / Cin); K chunks and row tiles of the packed form
    int row_ch, row_pos, col_ch, col_pos;      // nhwc_perm(channels, positions) of the rows / columns (channels 0: none)
    int vec, swizzle;                    // a lane's four source floats are one aligned float4; the 128-B-segment thread order (train_down.hip)
};
void launch_repack_down(const RepackDesc* table, int n, int blocks, const float* w, hipStream_t st);
// ... and of the generic path's packed forms, as k_repack_down_g rebuilds them (train_down_g.hip): RP_BIAS, RP_DENSE32, RP_DENSE16 and RP_CONV32
// as above, and three kinds of its own (an enum of its own: RepackKind is k_repack_down's)
enum RepackKindG {
    RP_CONVT32 = 8, // pack_conv (ConvTranspose2d, W [in][out][3][3]): nine taps of the 32x32x2 form
    RP_ENC1P,       // g_enc1p [9 taps][64 lanes][2] of qs_net.0.weight [32][in][3][3], zero for ci >= in; n = 1152 floats
    RP_WF4          // g_wf [9 taps][32][4] of po_net.19.weight [32][out][3][3], zero for c >= out; n = 1152 floats
};
void launch_repack_down_g(const RepackDesc* table, int n, int blocks, const float* w, hipStream_t st);

void launch_pack_x(const float* pi, const float* s, float* x, int R, int pi_dim, int s_dim, hipStream_t st);
void launch_pad16(const float* s, float* x, int R, int s_dim, hipStream_t st);
void launch_root_post(const float* enc, const float* pi, const float* eps_inj, float* x, float* s_out, int R, int use_mean,
                      uint32_t k0, uint32_t k1, uint32_t pass, uint32_t sample, uint32_t stage, uint32_t row_offset, int pi_dim, hipStream_t st);
void launch_root_post_rows(const float* enc, const float* pi, const float* eps_inj, float* x, float* s_out, int R, int use_mean,
                           uint32_t k0, uint32_t k1, uint32_t pass, uint32_t sample, uint32_t stage, uint32_t row_offset, int pi_dim,
                           const int32_t* ids, int ids_div, hipStream_t st);      // ids == nullptr: launch_root_post
void launch_split_enc(const float* enc, float* mean, float* logvar, int R, hipStream_t st);
void launch_softmax4(const float* logits32, float* logits, float* q, float* logq, int R, int n, hipStream_t st);
void launch_mean_rows(const float* G, float* out, int E, int T, hipStream_t st);
void launch_fill_tr(const float* mean, const float* logvar, float* tr, int R, hipStream_t st);
void launch_posterior(const float* sumG, float* P, float* logP, int n_groups, int n, float temperature, hipStream_t st);

void launch_check_reward(const float* o, float* out, int M, int intent, hipStream_t st);
void launch_reparam(const float* mean, const float* logvar, const float* eps_inj, float* out, int M, int n, uint32_t k0, uint32_t k1,
                    uint32_t pass, uint32_t sample, uint32_t stage, uint32_t row_offset, hipStream_t st);
void launch_env_step(float* state, float* last_r, const int* actions, int* round_changed, int E, int repeats,
                     uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, hipStream_t st);
void launch_env_new_image(float* state, int E, uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, hipStream_t st);
void launch_env_reset(float* state, float* last_r, int E, uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, hipStream_t st);
void launch_env_render(const float* state, const float* last_r, const unsigned char* imgs, long n_imgs, float* frames, int* err,
                       int E, hipStream_t st);

// ---- Dynamic-dSprites environment: what k_env_* (kernels.hip) and k_agent_act (agent.hip) share --------------------------------------
enum : uint32_t { TAG_ENV = 0x60, PASS_ENV = 9 };
__device__ __forceinline__ int env_randint(uint32_t k0, uint32_t k1, uint32_t game, uint32_t stage, int latent, int size) {
    const float u = u01(noise_words(k0, k1, TAG_ENV, (uint32_t)latent, game, stream_id(PASS_ENV, 0), stage).x);
    const int v = (int)(u * (float)size);
    return v < size ? v : size - 1;
}
// ONE tick of pi_to_action (game_environment.py:113-169) for one game: tick, move, and on a crossing the reward and new_image.
// s = the game's 7 state floats, r = its last_r (kept in a register by the caller); -> the round finished
__device__ __forceinline__ bool env_tick_move(float* s, float& r, int pi, uint32_t k0, uint32_t k1, uint32_t game, uint32_t stage) {
    bool changed = false;
    r *= 0.95f;                                                   // tick
    if (pi == 0) {                                                // up
        s[5] += 1.0f;
        if (s[5] >= 32.0f) {
            const float x = s[4];
            if (s[1] < 0.5f) r = (x > 15.0f) ? (15.0f - x) / 16.0f : (16.0f - x) / 16.0f;      // square
            else             r = (x > 15.0f) ? (x - 15.0f) / 16.0f : (x - 16.0f) / 16.0f;      // ellipse / heart
            const int sizes[6] = {1, 3, 6, 40, 32, 32};
            for (int k = 0; k < 6; ++k) s[k] = (float)env_randint(k0, k1, game, stage, k, sizes[k]);
            // port quirk, replicated because the oracle pins it: new_image() holds the accumulated reward as a tensor VIEW,
            // overwrites the row with a fresh sample (slot 6 = 0) and writes the view back -> the reward restarts at 0
            s[6] = 0.0f;
            changed = true;
        }
    } else if (pi == 1) { if (s[5] > 0.0f) s[5] -= 1.0f; }       // down
    else if (pi == 2) { if (s[4] < 31.0f) s[4] += 1.0f; }         // left
    else if (pi == 3) { if (s[4] > 0.0f) s[4] -= 1.0f; }          // right
    return changed;
}

// ---- agent control state (csrc/agent.hip; efe_agent of the C ABI) -------------------------------------------------------------------
struct AgentState { int32_t* queue; int32_t* head; int32_t* len; int32_t* crossings; float* reward_sum; int E, cap; };
enum : uint32_t { TAG_AGENT = 0x70 };                                // the action uniform of efe_agent_choose: word 0 of (TAG_AGENT, game, stream 0, stage)
enum { AGENT_AI = 0, AGENT_T1 = 1, AGENT_T12 = 2, AGENT_PROBS = 3 };
// The distribution an action is drawn from, for deciding game i of n (k_agent_choose draws from it, k_agent_trace_decision records it: one
// function, so the record holds the bits the draw used).  fp32 in the order of test_demo.py:152-159; see k_agent_choose for the formulas.
__device__ __forceinline__ void agent_probs(int mode, int i, int n, const float* sum_G, const float* sum_terms, const float* probs, int steps,
                                            float temperature, float p[4]) {
    if (mode == AGENT_PROBS) {
        for (int k = 0; k < 4; ++k) p[k] = probs[(size_t)i * 4 + k];
    } else {
        const float fs = (float)steps;
        float ex[4], sum = 0.f;
        for (int k = 0; k < 4; ++k) {
            const size_t r = (size_t)i * 4 + k;
            float x;
            if (mode == AGENT_AI) x = -(sum_G[r] / fs);
            else if (mode == AGENT_T1) x = sum_terms[r] / fs;
            else x = sum_terms[r] / fs - sum_terms[(size_t)n * 4 + r] / fs;
            ex[k] = expf(x / temperature);
            sum = (k == 0) ? ex[k] : sum + ex[k];
        }
        for (int k = 0; k < 4; ++k) p[k] = ex[k] / sum;
    }
}
void launch_agent_need(const AgentState& a, int32_t* ids, int32_t* count, hipStream_t st);
void launch_agent_choose(const AgentState& a, const int32_t* ids, int n, int mode, const float* sum_G, const float* sum_terms, const float* probs,
                         int steps, float temperature, int repeat, uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, const float* u,
                         int32_t* choice, float* u_out, hipStream_t st);
void launch_agent_enqueue(const AgentState& a, const int32_t* ids, int n, const int32_t* actions, const int32_t* lengths, int L, int jumps, hipStream_t st);
void launch_agent_act(const AgentState& a, float* state, float* last_r, int32_t* round_changed, uint32_t k0, uint32_t k1, uint32_t stage,
                      uint32_t game_offset, hipStream_t st);
// the two ends of an mcts decision (csrc/agent_mcts.hip): one thread per deciding slot i of game ids[i]; n < 1 launches nothing
void launch_agent_mcts_root(const AgentState& a, const int32_t* ids, int n, const float* Qpi, int A, int use_habit, float threshold, int jumps,
                            uint32_t k0, uint32_t k1, uint32_t stage, uint32_t game_offset, const float* u, uint8_t* active, uint8_t* decided,
                            int32_t* choice, float* u_out, hipStream_t st);
void launch_agent_mcts_enqueue(const AgentState& a, const MctsTree& t, const int32_t* ids, int n, const uint8_t* decided, int max_depth, int jumps,
                               int32_t* path_out, int32_t* path_len_out, hipStream_t st);
// the record of an agent run (csrc/agent_trace.hip; efe_agent_trace of the C ABI): T rows (ticks) x E games, row-major
struct AgentTrace { float* state; float* last_r; int32_t* action; int32_t* queue_len; uint8_t* decided; int32_t* choice; float* u; float* G;
                    float* terms; float* probs; int32_t* path; int32_t* path_len; int T, E, Lp; };
enum { AGENT_NONE = -1 };                                            // a decision without a recorded distribution (the slot planner's)
void launch_agent_trace_tick(const AgentState& a, const AgentTrace& tr, int row, const float* state, const float* last_r, hipStream_t st);
void launch_agent_trace_decision(const AgentTrace& tr, int row, const int32_t* ids, int n, int mode, const int32_t* choice, const float* u,
                                 const float* sum_G, const float* sum_terms, const float* probs, int steps, float temperature,
                                 const int32_t* path, const int32_t* path_len, int path_stride, hipStream_t st);
void launch_agent_plan_mask(const int32_t* ids, int n, int E, const float* state, const int32_t* H_act, const int32_t* H_len,
                            const uint8_t* H_active, int n_iter, int h_slots, int max_depth, int jumps, float* mask, hipStream_t st);
void launch_agent_view(const float* frames, const float* mask, const int32_t* ids, int n, int E, uint8_t* view, hipStream_t st);

}  // namespace efe
