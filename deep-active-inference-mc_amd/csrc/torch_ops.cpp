// torch.ops.efe.* : PyTorch-ROCm custom-op registration of the EFE engine, a thin layer over the C ABI of
// include/efe_engine.h.  Plain C++ (no device code): tensors in, tensors out; device memory comes from torch's allocator, the
// launch stream is torch's current HIP stream, errors become c10::Error (RuntimeError in Python).  The engine context is passed as
// an integer handle (the efe_ctx* returned by efe_create); its packed weights live in the context, not in the schema.
//
// Each op replaces one method of the reference's ActiveInferenceModel (/root/reference/src/torchmodel.py), cited per op.
// Only the CUDA (= HIP on ROCm) dispatch key is registered: calling an op with CPU tensors raises NotImplementedError -- there is
// no CPU fallback.
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include <string>
#include <tuple>
#include <vector>

#include "efe_engine.h"

#ifndef EFE_OPS_BUILD_ID
#define EFE_OPS_BUILD_ID "unstamped"
#endif
extern "C" const char* efe_ops_build_id(void) {
    static const char stamp[] = "EFE_OPS_BUILD_ID=" EFE_OPS_BUILD_ID;
    return stamp + 17;
}

namespace {

using at::Tensor;
using OptT = c10::optional<Tensor>;

bool given(const OptT& t) { return t.has_value() && t->defined(); }
float* P(const Tensor& t) { return t.data_ptr<float>(); }
const char* dtype_name(at::ScalarType ty) { return ty == at::kFloat ? "float32" : ty == at::kDouble ? "float64" : ty == at::kInt ? "int32" : "uint8"; }
int rows(const Tensor& t, int64_t width, const char* name) {
    TORCH_CHECK(t.numel() % width == 0 && t.numel() > 0, "efe: ", name, " must be [M, ", width, "]");
    return (int)(t.numel() / width);
}
efe_noise noise(int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset) {
    efe_noise nz;
    nz.seed = (uint64_t)seed; nz.stage = (uint32_t)stage; nz.pass = (uint32_t)pass; nz.sample = (uint32_t)sample;
    nz.row_offset = (uint32_t)row_offset;
    return nz;
}
efe_adam_params adam_params(double lr, double beta1, double beta2, double eps, int64_t step) {
    efe_adam_params hp;
    hp.lr = lr; hp.beta1 = beta1; hp.beta2 = beta2; hp.eps = eps; hp.step = step;
    return hp;
}
// the optional row set of a call (efe_rows): mask = uint8 [entries of the un-compacted batch], ids = int32 [entries of this call]
struct RowsArg {
    efe_rows r{nullptr, nullptr, 1, 0};
    Tensor mk, ik;
    bool set = false;
    const efe_rows* ptr() const { return set ? &r : nullptr; }
};

// One call's view of the engine context behind the integer handle.  The handle is checked against the engine's registry of live contexts
// (efe_ctx_alive: efe_create adds, efe_destroy removes), so a stale or made-up handle is a RuntimeError, not a dereference of freed memory.
// Every tensor of the call must live on the context's device (check() below): the launch stream is torch's current stream of THAT device.
struct Ctx {
    efe_ctx* c;
    int device = -1, s = 10, A = 4, C = 1, R = 64;      // efe_get_device, efe_get_config
    explicit Ctx(int64_t h) : c(reinterpret_cast<efe_ctx*>(static_cast<intptr_t>(h))) {
        TORCH_CHECK(h != 0, "efe: null engine context");
        TORCH_CHECK(efe_ctx_alive(c), "efe: stale or invalid engine context handle ", h, " (the context was destroyed, or this is not a handle of efe_create)");
        TORCH_CHECK(efe_get_device(c, &device, nullptr, 0) == 0, "efe: efe_get_device failed");
        efe_get_config(c, &s, &A, &C, &R);
    }
    int64_t img() const { return (int64_t)C * R * R; }
    void ok(int rc) const { TORCH_CHECK(rc == 0, "efe engine: ", efe_last_error(c)); }
    void* stream() const { return (void*)c10::hip::getCurrentHIPStream((c10::DeviceIndex)device).stream(); }
    int64_t param_count(const char* part) const {
        const int64_t n = efe_param_count(c, part);
        TORCH_CHECK(n > 0, "efe engine: ", efe_last_error(c));
        return n;
    }
    // the one device and dtype check: every tensor an op hands to the engine passes it
    const Tensor& check(const Tensor& t, const char* name, at::ScalarType ty = at::kFloat) const {
        TORCH_CHECK(t.is_cuda(), "efe: ", name, " must be a HIP device tensor (there is no CPU fallback)");
        TORCH_CHECK((int)t.device().index() == device, "efe: ", name, " is on device ", (int)t.device().index(), ", the engine context lives on device ",
                    device, " (one context per device: create the model on the tensor's device)");
        TORCH_CHECK(t.scalar_type() == ty, "efe: ", name, " must be ", dtype_name(ty));
        return t;
    }
    Tensor f32(const Tensor& t, const char* name) const { return check(t, name).contiguous(); }
    const float* opt(const OptT& t, Tensor& keep, const char* name, int64_t numel) const {
        if (!given(t)) return nullptr;
        keep = f32(*t, name);
        TORCH_CHECK(keep.numel() == numel, "efe: ", name, " has ", keep.numel(), " elements, expected ", numel);
        return P(keep);
    }
    // a tensor the call writes in place (optimiser state, a report row): contiguous float32 of n elements
    float* state(const Tensor& t, const char* name, int64_t n) const {
        TORCH_CHECK(check(t, name).is_contiguous() && t.numel() == n, "efe: ", name, " must be a contiguous float32 tensor of ", n, " elements");
        return P(t);
    }
    // the row set of a call of M rows in entries of rows_per_entry rows
    RowsArg row_set(const OptT& mask, const OptT& ids, int64_t rows_per_entry, int64_t M, int64_t n_total) const {
        RowsArg ra;
        TORCH_CHECK(rows_per_entry < 1 || M % rows_per_entry == 0, "efe: rows_per_entry must divide the row count");
        const bool hm = given(mask), hi = given(ids);
        if (!hm && !hi) return ra;
        TORCH_CHECK(rows_per_entry >= 1, "efe: rows_per_entry must be >= 1");
        const int64_t n_entries = M / rows_per_entry;
        ra.r.rows_per_entry = (int32_t)rows_per_entry;
        if (hm) {
            TORCH_CHECK(check(*mask, "row mask", at::kByte).is_contiguous(), "efe: row mask must be contiguous");
            TORCH_CHECK(hi || mask->numel() >= n_entries, "efe: row mask has ", mask->numel(), " entries, the call has ", n_entries);
            // the mask is indexed by entry ID: it must cover the whole un-compacted batch (n_total; with ids and no n_total the bound is unknown here)
            TORCH_CHECK(n_total <= 0 || mask->numel() >= n_total, "efe: row mask has ", mask->numel(), " entries, the un-compacted batch has ", n_total);
            if (n_total <= 0 && !hi) n_total = mask->numel();
            ra.mk = *mask; ra.r.mask = ra.mk.data_ptr<uint8_t>();
        }
        if (hi) {
            TORCH_CHECK(check(*ids, "row ids", at::kInt).is_contiguous(), "efe: row ids must be contiguous");
            TORCH_CHECK(ids->numel() == n_entries, "efe: row ids has ", ids->numel(), " entries, the call has ", n_entries);
            ra.ik = *ids; ra.r.ids = ra.ik.data_ptr<int32_t>();
        }
        TORCH_CHECK(n_total >= 0 && n_total <= INT32_MAX, "efe: bad n_total");
        ra.r.n_total = (int32_t)n_total;
        ra.set = true;
        return ra;
    }
};

// ModelMid.transition_with_sample, torchmodel.py:58-66
std::tuple<Tensor, Tensor, Tensor> transition(int64_t h, const Tensor& pi_, const Tensor& s0_, int64_t seed, int64_t stage, int64_t pass,
                                              int64_t sample, int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    Tensor pi = x.f32(pi_, "pi"), s0 = x.f32(s0_, "s0"), ek;
    const int M = rows(s0, 10, "s0");
    TORCH_CHECK(pi.numel() == (int64_t)M * x.A, "efe: pi must be [M, pi_dim]");
    Tensor ps1 = at::empty({M, 10}, s0.options()), mean = at::empty({M, 10}, s0.options()), lv = at::empty({M, 10}, s0.options());
    efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    x.ok(efe_transition(x.c, P(pi), P(s0), M, &nz, x.opt(eps, ek, "eps", (int64_t)M * 10), P(ps1), P(mean), P(lv), x.stream()));
    return {ps1, mean, lv};
}

// ModelDown.decoder, torchmodel.py:139-141
Tensor decoder(int64_t h, const Tensor& s_, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset) {
    Ctx x(h);
    Tensor s = x.f32(s_, "s");
    const int M = rows(s, 10, "s");
    Tensor po = at::empty({M, x.C, x.R, x.R}, s.options());
    efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    x.ok(efe_decoder(x.c, P(s), M, &nz, P(po), x.stream()));
    return po;
}

// ModelDown.encoder / encoder_with_sample, torchmodel.py:134-137, 143-146, over a row set (noise follows the entry id).  Without one the
// call is efe_encoder, with one efe_encoder_rows: the engine names the entry point in its messages
std::tuple<Tensor, Tensor, Tensor> encoder_rows(int64_t h, const Tensor& o_, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                                                int64_t row_offset, const OptT& eps, bool want_s, const OptT& mask, const OptT& ids,
                                                int64_t rows_per_entry, int64_t n_total) {
    Ctx x(h);
    Tensor o = x.f32(o_, "o"), ek;
    const int M = rows(o, x.img(), "o");
    Tensor s = want_s ? at::empty({M, 10}, o.options()) : at::empty({0}, o.options());
    Tensor mean = at::empty({M, 10}, o.options()), lv = at::empty({M, 10}, o.options());
    efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    const RowsArg ra = x.row_set(mask, ids, rows_per_entry, M, n_total);
    const float* e = x.opt(eps, ek, "eps", (int64_t)M * 10);
    float* sp = want_s ? P(s) : nullptr;
    x.ok(ra.set ? efe_encoder_rows(x.c, P(o), M, &nz, e, ra.ptr(), sp, P(mean), P(lv), x.stream())
                : efe_encoder(x.c, P(o), M, &nz, e, sp, P(mean), P(lv), x.stream()));
    return {s, mean, lv};
}
std::tuple<Tensor, Tensor, Tensor> encoder(int64_t h, const Tensor& o, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset,
                                           const OptT& eps, bool want_s) {
    return encoder_rows(h, o, seed, stage, pass, sample, row_offset, eps, want_s, c10::nullopt, c10::nullopt, 1, 0);
}

// ModelTop.encode_s, torchmodel.py:27-31
std::tuple<Tensor, Tensor, Tensor> habit(int64_t h, const Tensor& s_) {
    Ctx x(h);
    Tensor s = x.f32(s_, "s");
    const int M = rows(s, 10, "s");
    Tensor logits = at::empty({M, x.A}, s.options()), q = at::empty({M, x.A}, s.options()), logq = at::empty({M, x.A}, s.options());
    x.ok(efe_habit(x.c, P(s), M, P(logits), P(q), P(logq), x.stream()));
    return {logits, q, logq};
}

// calculate_G / calculate_G_mean, torchmodel.py:270-327
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> calculate_g(int64_t h, const Tensor& s0_, const Tensor& pi0_, int64_t samples,
                                                                       bool mean_mode, int64_t seed, int64_t stage, int64_t row_offset,
                                                                       const OptT& eps, const OptT& mask, const OptT& ids, int64_t rows_per_entry, int64_t n_total) {
    Ctx x(h);
    Tensor s0 = x.f32(s0_, "s0"), pi0 = x.f32(pi0_, "pi0"), ek;
    const int M = rows(s0, 10, "s0");
    TORCH_CHECK(pi0.numel() == (int64_t)M * x.A, "efe: pi0 must be [M, pi_dim]");
    TORCH_CHECK(samples >= 1 && samples <= 65535, "efe engine: samples must be in [1, 65535]");
    const int S = mean_mode ? 1 : (int)samples;
    auto op = s0.options();
    Tensor G = at::empty({M}, op), terms = at::empty({3, M}, op), ps1 = at::empty({M, 10}, op), ps1m = at::empty({M, 10}, op),
           po1 = at::empty({M, x.C, x.R, x.R}, op), parts = at::empty({2, M}, op);
    efe_noise nz = noise(seed, stage, 0, 0, row_offset);
    const RowsArg ra = x.row_set(mask, ids, rows_per_entry, M, n_total);
    x.ok(efe_calculate_g_rows(x.c, P(s0), P(pi0), M, S, mean_mode ? 1 : 0, &nz, x.opt(eps, ek, "eps", (int64_t)3 * S * M * 10), ra.ptr(), P(G), P(terms),
                              P(ps1), P(ps1m), P(po1), P(parts), x.stream()));
    return {G, terms, ps1, ps1m, po1, parts};
}

// calculate_G_repeated / calculate_G_4_repeated, torchmodel.py:227-268 (one row = one EFE rollout), over a row set: the rollouts of a
// compacted subset of the entries, noise keyed by the entry id.  Without one the call is efe_rollout, with one efe_rollout_rows
std::tuple<Tensor, Tensor, Tensor> rollout_rows(int64_t h, const Tensor& o_, const Tensor& pi_, int64_t steps, int64_t samples, bool calc_mean,
                                                bool per_stage_mean, int64_t seed, int64_t stage, int64_t row_offset, const OptT& eps,
                                                const OptT& mask, const OptT& ids, int64_t rows_per_entry, int64_t n_total) {
    Ctx x(h);
    Tensor o = x.f32(o_, "o"), pi = x.f32(pi_, "pi"), ek;
    const int M = rows(o, x.img(), "o");
    TORCH_CHECK(pi.numel() == (int64_t)M * x.A, "efe: o and pi must have the same number of rows");
    TORCH_CHECK(steps >= 1 && samples >= 1 && samples <= 65535, "efe engine: steps and samples must be >= 1");
    const int64_t S = (per_stage_mean && calc_mean) ? 1 : samples;
    auto op = o.options();
    Tensor G = at::empty({M}, op), terms = at::empty({3, M}, op), po1 = at::empty({M, x.C, x.R, x.R}, op);
    efe_noise nz = noise(seed, stage, 0, 0, row_offset);
    const RowsArg ra = x.row_set(mask, ids, rows_per_entry, M, n_total);
    const float* e = x.opt(eps, ek, "eps", (int64_t)M * 10 + steps * 3 * S * M * 10);
    const int cm = calc_mean ? 1 : 0, psm = per_stage_mean ? 1 : 0;
    x.ok(ra.set ? efe_rollout_rows(x.c, P(o), P(pi), M, (int)steps, (int)samples, cm, psm, &nz, e, ra.ptr(), P(G), P(terms), P(po1), x.stream())
                : efe_rollout(x.c, P(o), P(pi), M, (int)steps, (int)samples, cm, psm, &nz, e, P(G), P(terms), P(po1), x.stream()));
    return {G, terms, po1};
}
std::tuple<Tensor, Tensor, Tensor> rollout(int64_t h, const Tensor& o, const Tensor& pi, int64_t steps, int64_t samples, bool calc_mean, bool per_stage_mean,
                                           int64_t seed, int64_t stage, int64_t row_offset, const OptT& eps) {
    return rollout_rows(h, o, pi, steps, samples, calc_mean, per_stage_mean, seed, stage, row_offset, eps, c10::nullopt, c10::nullopt, 1, 0);
}

// calculate_G_given_trajectory, torchmodel.py:329-352
Tensor trajectory(int64_t h, const Tensor& s0_, const Tensor& ps1_, const Tensor& mean_, const Tensor& lv_, const Tensor& pi0_, int64_t seed,
                  int64_t stage, int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    Tensor s0 = x.f32(s0_, "s0_traj"), ps1 = x.f32(ps1_, "ps1_traj"), mean = x.f32(mean_, "ps1_mean_traj"), lv = x.f32(lv_, "ps1_logvar_traj"),
           pi0 = x.f32(pi0_, "pi0_traj"), ek;
    const int T = rows(s0, 10, "s0_traj");
    TORCH_CHECK(ps1.numel() == (int64_t)T * 10 && mean.numel() == (int64_t)T * 10 && lv.numel() == (int64_t)T * 10 && pi0.numel() == (int64_t)T * x.A,
                "efe: trajectory tensors must all have T rows");
    Tensor G = at::empty({T}, s0.options());
    efe_noise nz = noise(seed, stage, 0, 0, row_offset);
    x.ok(efe_trajectory(x.c, P(s0), P(ps1), P(mean), P(lv), P(pi0), T, &nz, x.opt(eps, ek, "eps", (int64_t)3 * T * 10), P(G), x.stream()));
    return G;
}

// mcts_step_simulate for E lock-step episodes, torchmodel.py:354-393
std::tuple<Tensor, Tensor, Tensor> simulate(int64_t h, const Tensor& s_, int64_t depth, bool use_means, int64_t seed, int64_t stage,
                                            int64_t row_offset, const OptT& eps, const OptT& u, const OptT& mask, const OptT& ids, int64_t n_total) {
    Ctx x(h);
    Tensor s = x.f32(s_, "starting_s"), ek, uk;
    const int E = rows(s, 10, "starting_s");
    TORCH_CHECK(depth >= 1 && depth <= 65535, "efe engine: depth must be in [1, 65535]");
    auto op = s.options();
    Tensor G = at::empty({E}, op), pi0 = at::empty({E, depth, x.A}, op), q0 = at::empty({E, x.A}, op);
    efe_noise nz = noise(seed, stage, 0, 0, row_offset);
    const RowsArg ra = x.row_set(mask, ids, 1, E, n_total);
    x.ok(efe_simulate_rows(x.c, P(s), E, (int)depth, use_means ? 1 : 0, &nz, x.opt(eps, ek, "eps", (int64_t)4 * depth * E * 10),
                           x.opt(u, uk, "u", depth * E), ra.ptr(), P(G), P(pi0), P(q0), x.stream()));
    return {G, pi0, q0};
}

// softmax_multi_with_log(-sum_G, n), /root/reference/src/util.py:46-53,68
std::tuple<Tensor, Tensor> action_posterior(int64_t h, const Tensor& g_, int64_t n, double temperature) {
    Ctx x(h);
    Tensor g = x.f32(g_, "sum_G");
    TORCH_CHECK(n >= 1 && n <= 8 && g.numel() % n == 0 && g.numel() > 0, "efe: sum_G must hold groups of n <= 8 values");
    const int64_t groups = g.numel() / n;
    Tensor Pr = at::empty({groups, n}, g.options()), logP = at::empty({groups, n}, g.options());
    x.ok(efe_action_posterior(x.c, P(g), (int)groups, (int)n, (float)temperature, P(Pr), P(logP), x.stream()));
    return {Pr, logP};
}

// ActiveInferenceModel.check_reward, torchmodel.py:210-212
Tensor check_reward(int64_t h, const Tensor& o_) {
    Ctx x(h);
    Tensor o = x.f32(o_, "o");
    const int M = rows(o, x.img(), "o");
    Tensor out = at::empty({M}, o.options());
    x.ok(efe_check_reward(x.c, P(o), M, P(out), x.stream()));
    return out;
}

// Model{Mid,Down}.reparameterize, torchmodel.py:54-56 / 130-132
Tensor reparameterize(int64_t h, const Tensor& mean_, const Tensor& lv_, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                      int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    Tensor mean = x.f32(mean_, "mean"), lv = x.f32(lv_, "logvar"), ek;
    TORCH_CHECK(mean.dim() == 2 && mean.sizes() == lv.sizes(), "efe: mean and logvar must be [M, n]");
    const int M = (int)mean.size(0), n = (int)mean.size(1);
    Tensor out = at::empty({M, n}, mean.options());
    efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    x.ok(efe_reparameterize(x.c, P(mean), P(lv), M, n, &nz, x.opt(eps, ek, "eps", (int64_t)M * n), P(out), x.stream()));
    return out;
}

// ---- training-side free energy, forward (/root/reference/src/torchloss.py) ----
efe_fe_params fe_params(const Ctx& x, double gamma, double beta_s, double beta_o, int64_t omega_mode, const OptT& omega, Tensor& keep,
                        double omega_scalar, int64_t M) {
    efe_fe_params p{};
    p.gamma = (float)gamma; p.beta_s = (float)beta_s; p.beta_o = (float)beta_o; p.omega_mode = (int32_t)omega_mode;
    p.omega = x.opt(omega, keep, "omega", M); p.omega_scalar = (float)omega_scalar;
    TORCH_CHECK(omega_mode != EFE_OMEGA_ARRAY || p.omega, "efe: omega_mode 0 (per-row omega) needs an omega tensor of M elements");
    return p;
}

// The argument bundles of the training-side ops: the inputs of one reference function, checked once, with the parameter block, the noise
// keys and the injected normals that go with them.  Each is shared by the forward op, the gradient op and the training op of its part.
// (s, log_Ppi) of compute_loss_top
struct TopIn { Tensor s, lp; int M; };
TopIn top_in(const Ctx& x, const Tensor& s_, const Tensor& lp_) {
    TopIn r{x.f32(s_, "s"), x.f32(lp_, "log_Ppi"), 0};
    r.M = rows(r.s, 10, "s");
    TORCH_CHECK(r.lp.numel() == (int64_t)r.M * x.A, "efe: log_Ppi must be [M, pi_dim]");
    return r;
}
// the inputs of compute_loss_mid
struct MidIn { Tensor s0, pi0, qm, qv, keep; int M; efe_fe_params p; efe_noise nz; };
MidIn mid_in(const Ctx& x, const Tensor& s0_, const Tensor& pi0_, const Tensor& qm_, const Tensor& qv_, int64_t omega_mode, const OptT& omega,
             double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset) {
    MidIn r;
    r.s0 = x.f32(s0_, "s0"); r.pi0 = x.f32(pi0_, "Ppi_sampled"); r.qm = x.f32(qm_, "qs1_mean"); r.qv = x.f32(qv_, "qs1_logvar");
    r.M = rows(r.s0, 10, "s0");
    TORCH_CHECK(r.pi0.numel() == (int64_t)r.M * x.A, "efe: Ppi_sampled must be [M, pi_dim]");
    TORCH_CHECK(r.qm.numel() == (int64_t)r.M * 10 && r.qv.numel() == (int64_t)r.M * 10, "efe: qs1_mean and qs1_logvar must be [M, 10]");
    r.p = fe_params(x, 0.0, 0.0, 0.0, omega_mode, omega, r.keep, omega_scalar, r.M);
    r.nz = noise(seed, stage, pass, sample, row_offset);
    return r;
}
// the inputs of compute_loss_down
struct DownIn { Tensor o1, pm, pv, keep, ek; int M; efe_fe_params p; efe_noise nz; const float* eps; };
DownIn down_in(const Ctx& x, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
               const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset, const OptT& eps) {
    DownIn r;
    r.o1 = x.f32(o1_, "o1"); r.pm = x.f32(pm_, "ps1_mean"); r.pv = x.f32(pv_, "ps1_logvar");
    r.M = rows(r.o1, x.img(), "o1");
    TORCH_CHECK(r.pm.numel() == (int64_t)r.M * 10 && r.pv.numel() == (int64_t)r.M * 10, "efe: ps1_mean and ps1_logvar must be [M, 10]");
    r.p = fe_params(x, gamma, beta_s, beta_o, omega_mode, omega, r.keep, omega_scalar, r.M);
    r.nz = noise(seed, stage, pass, sample, row_offset);
    r.eps = x.opt(eps, r.ek, "eps", (int64_t)r.M * 10);
    return r;
}
// the inputs of one whole step, train.py:104-123: both frames, the action and its prior, compute_omega's a..d, normals [3][M][s_dim]
struct StepIn { Tensor o0, o1, pi0, lp, keep, ek; int M; efe_fe_params p; efe_noise nz; const float* eps; };
StepIn step_in(const Ctx& x, const Tensor& o0_, const Tensor& o1_, const Tensor& pi0_, const Tensor& lp_, double gamma, double beta_s, double beta_o,
               int64_t omega_mode, const OptT& omega, double omega_scalar, double a, double b, double cc, double d, int64_t seed, int64_t stage,
               int64_t row_offset, const OptT& eps) {
    StepIn r;
    r.o0 = x.f32(o0_, "o0"); r.o1 = x.f32(o1_, "o1"); r.pi0 = x.f32(pi0_, "pi0"); r.lp = x.f32(lp_, "log_Ppi");
    r.M = rows(r.o0, x.img(), "o0");
    TORCH_CHECK(r.o1.numel() == (int64_t)r.M * x.img(), "efe: o1 must have the shape of o0");
    TORCH_CHECK(r.pi0.numel() == (int64_t)r.M * x.A && r.lp.numel() == (int64_t)r.M * x.A, "efe: pi0 and log_Ppi must be [M, pi_dim]");
    r.p = fe_params(x, gamma, beta_s, beta_o, omega_mode, omega, r.keep, omega_scalar, r.M);
    r.p.a = (float)a; r.p.b = (float)b; r.p.c = (float)cc; r.p.d = (float)d;
    r.nz = noise(seed, stage, 0, 0, row_offset);
    r.eps = x.opt(eps, r.ek, "eps", (int64_t)3 * r.M * x.s);
    return r;
}

// ActiveInferenceModel training step, train.py:104-123 (compute_loss_top / _mid / _down composed); outputs in efe_fe_out order
std::vector<Tensor> free_energy(int64_t h, const Tensor& o0_, const Tensor& o1_, const Tensor& pi0_, const Tensor& lp_, double gamma, double beta_s,
                                double beta_o, int64_t omega_mode, const OptT& omega, double omega_scalar, double a, double b, double cc, double d,
                                int64_t seed, int64_t stage, int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    StepIn in = step_in(x, o0_, o1_, pi0_, lp_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, a, b, cc, d, seed, stage, row_offset, eps);
    auto op = in.o0.options();
    const int64_t M = in.M, S = x.s, A = x.A;
    std::vector<Tensor> r = {
        at::empty({M}, op), at::empty({M}, op), at::empty({M, A}, op), at::empty({M, A}, op), at::empty({M}, op),
        at::empty({M}, op), at::empty({M}, op), at::empty({M, S}, op), at::empty({M, S}, op), at::empty({M, S}, op), at::empty({M, S}, op),
        at::empty({M}, op), at::empty({M}, op), at::empty({M}, op), at::empty({M, S}, op), at::empty({M}, op), at::empty({M, S}, op),
        at::empty({M, x.C, x.R, x.R}, op), at::empty({M, S}, op), at::empty({M, S}, op), at::empty({M, S}, op), at::empty({M, S}, op)};
    efe_fe_out out{P(r[0]), P(r[1]), P(r[2]), P(r[3]), P(r[4]), P(r[5]), P(r[6]), P(r[7]), P(r[8]), P(r[9]), P(r[10]), P(r[11]), P(r[12]),
                   P(r[13]), P(r[14]), P(r[15]), P(r[16]), P(r[17]), P(r[18]), P(r[19]), P(r[20]), P(r[21])};
    x.ok(efe_free_energy(x.c, P(in.o0), P(in.o1), P(in.pi0), P(in.lp), in.M, &in.p, &in.nz, in.eps, &out, x.stream()));
    return r;
}

// compute_loss_top, torchloss.py:19-26
std::tuple<Tensor, Tensor, Tensor, Tensor> loss_top(int64_t h, const Tensor& s_, const Tensor& lp_) {
    Ctx x(h);
    TopIn in = top_in(x, s_, lp_);
    auto op = in.s.options();
    Tensor F = at::empty({in.M}, op), kl = at::empty({in.M}, op), anal = at::empty({in.M, x.A}, op), q = at::empty({in.M, x.A}, op);
    efe_fe_out out{};
    out.F_top = P(F); out.kl_pi = P(kl); out.kl_pi_anal = P(anal); out.Qpi = P(q);
    x.ok(efe_loss_top(x.c, P(in.s), P(in.lp), in.M, &out, x.stream()));
    return {F, kl, anal, q};
}

// compute_loss_mid, torchloss.py:28-36
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> loss_mid(int64_t h, const Tensor& s0_, const Tensor& pi0_, const Tensor& qm_, const Tensor& qv_,
                                                                    int64_t omega_mode, const OptT& omega, double omega_scalar, int64_t seed,
                                                                    int64_t stage, int64_t pass, int64_t sample, int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    MidIn a = mid_in(x, s0_, pi0_, qm_, qv_, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset);
    auto op = a.s0.options();
    Tensor F = at::empty({a.M}, op), kl = at::empty({a.M}, op), anal = at::empty({a.M, 10}, op), ps1 = at::empty({a.M, 10}, op),
           pm = at::empty({a.M, 10}, op), pv = at::empty({a.M, 10}, op), ek;
    efe_fe_out out{};
    out.F_mid = P(F); out.kl_s_mid = P(kl); out.kl_s_mid_anal = P(anal); out.ps1 = P(ps1); out.ps1_mean = P(pm); out.ps1_logvar = P(pv);
    x.ok(efe_loss_mid(x.c, P(a.s0), P(a.pi0), P(a.qm), P(a.qv), a.M, &a.p, &a.nz, x.opt(eps, ek, "eps", (int64_t)a.M * 10), &out, x.stream()));
    return {F, kl, anal, ps1, pm, pv};
}

// compute_loss_down, torchloss.py:53-74
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> loss_down(
        int64_t h, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
        const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset, const OptT& eps) {
    Ctx x(h);
    DownIn in = down_in(x, o1_, pm_, pv_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset, eps);
    auto op = in.o1.options();
    const int64_t M = in.M;
    Tensor F = at::empty({M}, op), nl = at::empty({M}, op), kls = at::empty({M}, op), klsa = at::empty({M, 10}, op), kln = at::empty({M}, op),
           klna = at::empty({M, 10}, op), po1 = at::empty({M, x.C, x.R, x.R}, op), qs1 = at::empty({M, 10}, op);
    efe_fe_out out{};
    out.F_down = P(F); out.nlogpo1 = P(nl); out.kl_s = P(kls); out.kl_s_anal = P(klsa); out.kl_naive = P(kln); out.kl_naive_anal = P(klna);
    out.po1 = P(po1); out.qs1 = P(qs1);
    x.ok(efe_loss_down(x.c, P(in.o1), P(in.pm), P(in.pv), in.M, &in.p, &in.nz, in.eps, &out, x.stream()));
    return {F, nl, kls, klsa, kln, klna, po1, qs1};
}

// ---- training of the habit net (csrc/train.hip) ----
// d mean(F_top) / d qpi_net parameters (torchloss.py:65-72 up to optimizer.step) -> (kl_pi [M], grad [P])
std::tuple<Tensor, Tensor> top_grad(int64_t h, const Tensor& s_, const Tensor& lp_) {
    Ctx x(h);
    TopIn in = top_in(x, s_, lp_);
    Tensor kl = at::empty({in.M}, in.s.options()), grad = at::empty({x.param_count("top")}, in.s.options());
    x.ok(efe_top_grad(x.c, P(in.s), P(in.lp), in.M, P(kl), P(grad), x.stream()));
    return {kl, grad};
}

// torch.optim.Adam.step() of one part with the caller's gradient and state
void adam_step(int64_t h, c10::string_view part, const Tensor& grad_, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2,
               double eps, int64_t step) {
    Ctx x(h);
    const std::string pt(part);
    const int64_t NP = x.param_count(pt.c_str());
    Tensor grad = x.f32(grad_, "grad");
    TORCH_CHECK(grad.numel() == NP, "efe: grad has ", grad.numel(), " elements, the part has ", NP, " parameters");
    const efe_adam_params hp = adam_params(lr, beta1, beta2, eps, step);
    x.ok(efe_adam_step(x.c, pt.c_str(), P(grad), x.state(exp_avg, "exp_avg", NP), x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
}

// train_model_top, torchloss.py:65-74 -> kl_pi [M] of the weights before the step
Tensor train_top(int64_t h, const Tensor& s_, const Tensor& lp_, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps,
                 int64_t step) {
    Ctx x(h);
    TopIn in = top_in(x, s_, lp_);
    const int64_t NP = x.param_count("top");
    Tensor kl = at::empty({in.M}, in.s.options());
    const efe_adam_params hp = adam_params(lr, beta1, beta2, eps, step);
    x.ok(efe_train_top(x.c, P(in.s), P(in.lp), in.M, P(kl), x.state(exp_avg, "exp_avg", NP), x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
    return kl;
}

// ---- training of the transition net (csrc/train.hip k_mid_grad) ----
// d mean(F_mid) / d ps_net parameters (torchloss.py:76-86 up to optimizer.step) -> (F_mid [M], ps1_mean, ps1_logvar [M,10], grad [P])
std::tuple<Tensor, Tensor, Tensor, Tensor> mid_grad(int64_t h, const Tensor& s0_, const Tensor& pi0_, const Tensor& qm_, const Tensor& qv_, int64_t omega_mode,
                                                    const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                                                    int64_t row_offset) {
    Ctx x(h);
    MidIn a = mid_in(x, s0_, pi0_, qm_, qv_, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset);
    auto op = a.s0.options();
    Tensor F = at::empty({a.M}, op), pm = at::empty({a.M, 10}, op), pv = at::empty({a.M, 10}, op), grad = at::empty({x.param_count("ps_net")}, op);
    x.ok(efe_mid_grad(x.c, P(a.s0), P(a.pi0), P(a.qm), P(a.qv), a.M, &a.p, &a.nz, P(pm), P(pv), P(F), P(grad), x.stream()));
    return {F, pm, pv, grad};
}

// train_model_mid, torchloss.py:76-88 -> (ps1_mean, ps1_logvar, F_mid) of the weights before the step
std::tuple<Tensor, Tensor, Tensor> train_mid(int64_t h, const Tensor& s0_, const Tensor& pi0_, const Tensor& qm_, const Tensor& qv_, int64_t omega_mode,
                                             const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                                             int64_t row_offset, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps,
                                             int64_t step) {
    Ctx x(h);
    MidIn a = mid_in(x, s0_, pi0_, qm_, qv_, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset);
    const int64_t NP = x.param_count("ps_net");
    auto op = a.s0.options();
    Tensor F = at::empty({a.M}, op), pm = at::empty({a.M, 10}, op), pv = at::empty({a.M, 10}, op);
    const efe_adam_params hp = adam_params(lr, beta1, beta2, eps, step);
    x.ok(efe_train_mid(x.c, P(a.s0), P(a.pi0), P(a.qm), P(a.qv), a.M, &a.p, &a.nz, P(pm), P(pv), P(F), x.state(exp_avg, "exp_avg", NP),
                       x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
    return {pm, pv, F};
}

// ---- backward of the decoder's ConvTranspose2d tail (csrc/train_dec.hip) ----
// d (scale * sum nlogpo1) / d (po_net.13 .. 19, h4) -> (nlogpo1 [M], po1 [M,1,64,64], d_h4 [M,16384], grad [92609], y1, y2, y3); the
// activations are empty tensors unless want_y; scale < 0: beta_o / M
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> dec_tail_grad(int64_t h, const Tensor& h4_, const Tensor& o1_, double scale, double beta_o,
                                                                                  bool want_y) {
    Ctx x(h);
    Tensor h4 = x.f32(h4_, "h4"), o1 = x.f32(o1_, "o1");
    const int M = rows(h4, 16384, "h4");
    TORCH_CHECK(o1.numel() == (int64_t)M * 4096, "efe: o1 must be [M, 1, 64, 64]");
    const int64_t NP = x.param_count("po_net_convt");
    auto op = h4.options();
    const int64_t My = want_y ? M : 0;
    Tensor nl = at::empty({M}, op), po = at::empty({M, 1, 64, 64}, op), dh = at::empty({M, 16384}, op), grad = at::empty({NP}, op);
    Tensor y1 = at::empty({My, 64, 16, 16}, op), y2 = at::empty({My, 64, 32, 32}, op), y3 = at::empty({My, 32, 64, 64}, op);
    auto A = [&](Tensor& t) { return want_y ? P(t) : nullptr; };
    x.ok(efe_dec_tail_grad(x.c, P(h4), P(o1), M, (float)scale, (float)beta_o, P(nl), P(po), P(dh), P(grad), A(y1), A(y2), A(y3), x.stream()));
    return {nl, po, dh, grad, y1, y2, y3};
}

// ---- the same at every admitted geometry (csrc/train_dec_g.hip): sizes from the context ----
// -> (nlogpo1 [M], po1 [M,C,R,R], d_h4 [M,64 B B], grad [92320 + 289 C], y1 [M,64,B,B], y2 [M,64,2B,2B], y3 [M,32,R,R])
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> dec_tail_grad_g(int64_t h, const Tensor& h4_, const Tensor& o1_, double scale, double beta_o,
                                                                                    bool want_y) {
    Ctx x(h);
    Tensor h4 = x.f32(h4_, "h4"), o1 = x.f32(o1_, "o1");
    const int64_t R = x.R, B = R == 32 ? 16 : R / 4, C = x.C;
    const int M = rows(h4, 64 * B * B, "h4");
    TORCH_CHECK(o1.numel() == (int64_t)M * x.img(), "efe: o1 must be [M, ", C, ", ", R, ", ", R, "]");
    const int64_t NP = x.param_count("po_net_convt");
    auto op = h4.options();
    const int64_t My = want_y ? M : 0;
    Tensor nl = at::empty({M}, op), po = at::empty({M, C, R, R}, op), dh = at::empty({M, 64 * B * B}, op), grad = at::empty({NP}, op);
    Tensor y1 = at::empty({My, 64, B, B}, op), y2 = at::empty({My, 64, 2 * B, 2 * B}, op), y3 = at::empty({My, 32, R, R}, op);
    auto A = [&](Tensor& t) { return want_y ? P(t) : nullptr; };
    x.ok(efe_dec_tail_grad_g(x.c, P(h4), P(o1), M, (float)scale, (float)beta_o, P(nl), P(po), P(dh), P(grad), A(y1), A(y2), A(y3), x.stream()));
    return {nl, po, dh, grad, y1, y2, y3};
}

// ---- backward of the whole decoder (csrc/train_dec_head.hip + csrc/train_dec.hip) ----
// d (scale * sum nlogpo1) / d (po_net, s) -> (nlogpo1 [M], po1 [M,1,64,64], d_s [M,10], grad [4437697], h1, h2, h3, h4, y1, y2, y3); the
// activations are empty tensors unless want_act; scale < 0: beta_o / M
std::vector<Tensor> dec_grad(int64_t h, const Tensor& s_, const Tensor& o1_, double scale, double beta_o, int64_t seed, int64_t stage, int64_t pass,
                             int64_t sample, int64_t row_offset, bool want_act) {
    Ctx x(h);
    Tensor s = x.f32(s_, "s"), o1 = x.f32(o1_, "o1");
    const int M = rows(s, 10, "s");
    TORCH_CHECK(o1.numel() == (int64_t)M * 4096, "efe: o1 must be [M, 1, 64, 64]");
    const int64_t NP = x.param_count("po_net");
    const efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    auto op = s.options();
    const int64_t Ma = want_act ? M : 0;
    Tensor nl = at::empty({M}, op), po = at::empty({M, 1, 64, 64}, op), ds = at::empty({M, 10}, op), grad = at::empty({NP}, op);
    Tensor h1 = at::empty({Ma, 256}, op), h2 = at::empty({Ma, 256}, op), h3 = at::empty({Ma, 256}, op), h4 = at::empty({Ma, 16384}, op);
    Tensor y1 = at::empty({Ma, 64, 16, 16}, op), y2 = at::empty({Ma, 64, 32, 32}, op), y3 = at::empty({Ma, 32, 64, 64}, op);
    auto A = [&](Tensor& t) { return want_act ? P(t) : nullptr; };
    x.ok(efe_dec_grad(x.c, P(s), P(o1), M, (float)scale, (float)beta_o, &nz, P(nl), P(po), P(ds), P(grad), A(h1), A(h2), A(h3), A(h4), A(y1), A(y2),
                      A(y3), x.stream()));
    return {nl, po, ds, grad, h1, h2, h3, h4, y1, y2, y3};
}

// ---- the same at every admitted geometry (csrc/train_dec_head_g.hip + csrc/train_dec_g.hip): sizes from the context ----
// -> (nlogpo1 [M], po1 [M,C,R,R], d_s [M,10], grad [134400 + 257 F + 92320 + 289 C], h1, h2, h3 [M,256], h4 [M,F], y1, y2, y3), F = 64 B B
std::vector<Tensor> dec_grad_g(int64_t h, const Tensor& s_, const Tensor& o1_, double scale, double beta_o, int64_t seed, int64_t stage, int64_t pass,
                               int64_t sample, int64_t row_offset, bool want_act) {
    Ctx x(h);
    Tensor s = x.f32(s_, "s"), o1 = x.f32(o1_, "o1");
    const int64_t R = x.R, B = R == 32 ? 16 : R / 4, C = x.C;
    const int M = rows(s, 10, "s");
    TORCH_CHECK(o1.numel() == (int64_t)M * x.img(), "efe: o1 must be [M, ", C, ", ", R, ", ", R, "]");
    const int64_t NP = x.param_count("po_net");
    const efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    auto op = s.options();
    const int64_t Ma = want_act ? M : 0;
    Tensor nl = at::empty({M}, op), po = at::empty({M, C, R, R}, op), ds = at::empty({M, 10}, op), grad = at::empty({NP}, op);
    Tensor h1 = at::empty({Ma, 256}, op), h2 = at::empty({Ma, 256}, op), h3 = at::empty({Ma, 256}, op), h4 = at::empty({Ma, 64 * B * B}, op);
    Tensor y1 = at::empty({Ma, 64, B, B}, op), y2 = at::empty({Ma, 64, 2 * B, 2 * B}, op), y3 = at::empty({Ma, 32, R, R}, op);
    auto A = [&](Tensor& t) { return want_act ? P(t) : nullptr; };
    x.ok(efe_dec_grad_g(x.c, P(s), P(o1), M, (float)scale, (float)beta_o, &nz, P(nl), P(po), P(ds), P(grad), A(h1), A(h2), A(h3), A(h4), A(y1), A(y2),
                        A(y3), x.stream()));
    return {nl, po, ds, grad, h1, h2, h3, h4, y1, y2, y3};
}

// ---- backward of the encoder (csrc/train_enc.hip) ----
// the vector-Jacobian product of qs_net for (g_mean, g_logvar) -> (mean [M,10], logvar [M,10], grad [349428], y1, y2, y3, y4, h1, h2, h3); the
// activations are empty tensors unless want_act
std::vector<Tensor> enc_grad(int64_t h, const Tensor& o_, const Tensor& gm_, const Tensor& gv_, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                             int64_t row_offset, bool want_act) {
    Ctx x(h);
    Tensor o = x.f32(o_, "o"), gm = x.f32(gm_, "d_mean"), gv = x.f32(gv_, "d_logvar");
    const int M = rows(o, 4096, "o");
    TORCH_CHECK(gm.numel() == (int64_t)M * 10 && gv.numel() == (int64_t)M * 10, "efe: d_mean and d_logvar must be [M, 10]");
    const int64_t NP = x.param_count("qs_net");
    const efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    auto op = o.options();
    const int64_t Ma = want_act ? M : 0;
    Tensor mean = at::empty({M, 10}, op), lv = at::empty({M, 10}, op), grad = at::empty({NP}, op);
    Tensor y1 = at::empty({Ma, 32, 31, 31}, op), y2 = at::empty({Ma, 32, 15, 15}, op), y3 = at::empty({Ma, 64, 7, 7}, op), y4 = at::empty({Ma, 64, 3, 3}, op);
    Tensor h1 = at::empty({Ma, 256}, op), h2 = at::empty({Ma, 256}, op), h3 = at::empty({Ma, 256}, op);
    auto A = [&](Tensor& t) { return want_act ? P(t) : nullptr; };
    x.ok(efe_enc_grad(x.c, P(o), P(gm), P(gv), M, &nz, P(mean), P(lv), P(grad), A(y1), A(y2), A(y3), A(y4), A(h1), A(h2), A(h3), x.stream()));
    return {mean, lv, grad, y1, y2, y3, y4, h1, h2, h3};
}

// ---- gradient of F_down for all of ModelDown (csrc/train_enc.hip + the decoder's two files) ----
// -> (F_down [M], nlogpo1 [M], kl_s [M], kl_naive [M], po1 [M,1,64,64], qs1, qs1_mean, qs1_logvar [M,10], g_mean, g_logvar [M,10], grad [4787125])
std::vector<Tensor> down_grad(int64_t h, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
                              const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset,
                              const OptT& eps) {
    Ctx x(h);
    const int64_t NP = x.param_count("down");
    DownIn in = down_in(x, o1_, pm_, pv_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset, eps);
    auto op = in.o1.options();
    const int64_t M = in.M;
    Tensor F = at::empty({M}, op), nl = at::empty({M}, op), kls = at::empty({M}, op), kln = at::empty({M}, op), po1 = at::empty({M, 1, 64, 64}, op);
    Tensor qs1 = at::empty({M, 10}, op), qm = at::empty({M, 10}, op), qv = at::empty({M, 10}, op), gm = at::empty({M, 10}, op), gv = at::empty({M, 10}, op);
    Tensor grad = at::empty({NP}, op);
    efe_fe_out out{};
    out.F_down = P(F); out.nlogpo1 = P(nl); out.kl_s = P(kls); out.kl_naive = P(kln); out.po1 = P(po1); out.qs1 = P(qs1);
    out.qs1_mean = P(qm); out.qs1_logvar = P(qv);
    x.ok(efe_down_grad(x.c, P(in.o1), P(in.pm), P(in.pv), in.M, &in.p, &in.nz, in.eps, &out, P(gm), P(gv), P(grad), x.stream()));
    return {F, nl, kls, kln, po1, qs1, qm, qv, gm, gv, grad};
}

// ---- the same two at every admitted geometry (csrc/train_enc_g.hip): sizes from the context ----
// -> (mean [M,10], logvar [M,10], grad [201684 + 288 C + 256 K], y1 [M,32,H1,H1], y2 [M,32,H2,H2], y3 [M,64,H3,H3], y4 [M,64,H4,H4], h1, h2, h3 [M,256]),
// H_l = (H_{l-1} - 3) / 2 + 1 from R, K = 64 H4 H4
std::vector<Tensor> enc_grad_g(int64_t h, const Tensor& o_, const Tensor& gm_, const Tensor& gv_, int64_t seed, int64_t stage, int64_t pass, int64_t sample,
                               int64_t row_offset, bool want_act) {
    Ctx x(h);
    Tensor o = x.f32(o_, "o"), gm = x.f32(gm_, "d_mean"), gv = x.f32(gv_, "d_logvar");
    const int M = rows(o, x.img(), "o");
    TORCH_CHECK(gm.numel() == (int64_t)M * 10 && gv.numel() == (int64_t)M * 10, "efe: d_mean and d_logvar must be [M, 10]");
    const int64_t NP = x.param_count("qs_net_g");
    const efe_noise nz = noise(seed, stage, pass, sample, row_offset);
    auto op = o.options();
    const int64_t Ma = want_act ? M : 0;
    const int64_t H1 = (x.R - 3) / 2 + 1, H2 = (H1 - 3) / 2 + 1, H3 = (H2 - 3) / 2 + 1, H4 = (H3 - 3) / 2 + 1;
    Tensor mean = at::empty({M, 10}, op), lv = at::empty({M, 10}, op), grad = at::empty({NP}, op);
    Tensor y1 = at::empty({Ma, 32, H1, H1}, op), y2 = at::empty({Ma, 32, H2, H2}, op), y3 = at::empty({Ma, 64, H3, H3}, op), y4 = at::empty({Ma, 64, H4, H4}, op);
    Tensor h1 = at::empty({Ma, 256}, op), h2 = at::empty({Ma, 256}, op), h3 = at::empty({Ma, 256}, op);
    auto A = [&](Tensor& t) { return want_act ? P(t) : nullptr; };
    x.ok(efe_enc_grad_g(x.c, P(o), P(gm), P(gv), M, &nz, P(mean), P(lv), P(grad), A(y1), A(y2), A(y3), A(y4), A(h1), A(h2), A(h3), x.stream()));
    return {mean, lv, grad, y1, y2, y3, y4, h1, h2, h3};
}

// -> (F_down [M], nlogpo1 [M], kl_s [M], kl_naive [M], po1 [M,C,R,R], qs1, qs1_mean, qs1_logvar [M,10], g_mean, g_logvar [M,10], grad [qs_net then po_net])
std::vector<Tensor> down_grad_g(int64_t h, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
                                const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset,
                                const OptT& eps) {
    Ctx x(h);
    const int64_t NP = x.param_count("down_g");
    DownIn in = down_in(x, o1_, pm_, pv_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset, eps);
    auto op = in.o1.options();
    const int64_t M = in.M;
    Tensor F = at::empty({M}, op), nl = at::empty({M}, op), kls = at::empty({M}, op), kln = at::empty({M}, op), po1 = at::empty({M, x.C, x.R, x.R}, op);
    Tensor qs1 = at::empty({M, 10}, op), qm = at::empty({M, 10}, op), qv = at::empty({M, 10}, op), gm = at::empty({M, 10}, op), gv = at::empty({M, 10}, op);
    Tensor grad = at::empty({NP}, op);
    efe_fe_out out{};
    out.F_down = P(F); out.nlogpo1 = P(nl); out.kl_s = P(kls); out.kl_naive = P(kln); out.po1 = P(po1); out.qs1 = P(qs1);
    out.qs1_mean = P(qm); out.qs1_logvar = P(qv);
    x.ok(efe_down_grad_g(x.c, P(in.o1), P(in.pm), P(in.pv), in.M, &in.p, &in.nz, in.eps, &out, P(gm), P(gv), P(grad), x.stream()));
    return {F, nl, kls, kln, po1, qs1, qm, qv, gm, gv, grad};
}

// train_model_down, torchloss.py:90-98 (csrc/train_down.hip behind the gradient) -> (F_down, nlogpo1, kl_s, kl_naive [M]) of the weights before the step
std::vector<Tensor> train_down(int64_t h, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
                               const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset,
                               const OptT& eps, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double aeps, int64_t step) {
    Ctx x(h);
    const int64_t NP = x.param_count("down");
    DownIn in = down_in(x, o1_, pm_, pv_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset, eps);
    auto op = in.o1.options();
    const int64_t M = in.M;
    Tensor F = at::empty({M}, op), nl = at::empty({M}, op), kls = at::empty({M}, op), kln = at::empty({M}, op);
    efe_fe_out out{};
    out.F_down = P(F); out.nlogpo1 = P(nl); out.kl_s = P(kls); out.kl_naive = P(kln);
    const efe_adam_params hp = adam_params(lr, beta1, beta2, aeps, step);
    x.ok(efe_train_down(x.c, P(in.o1), P(in.pm), P(in.pv), in.M, &in.p, &in.nz, in.eps, &out, x.state(exp_avg, "exp_avg", NP),
                        x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
    return {F, nl, kls, kln};
}

// torch.optim.Adam.step() of ModelDown with the caller's gradient and state, and the packed forward forms rebuilt
void down_adam_step(int64_t h, const Tensor& grad_, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step) {
    Ctx x(h);
    const int64_t NP = x.param_count("down");
    Tensor grad = x.f32(grad_, "grad");
    TORCH_CHECK(grad.numel() == NP, "efe: grad has ", grad.numel(), " elements, ModelDown has ", NP, " parameters");
    const efe_adam_params hp = adam_params(lr, beta1, beta2, eps, step);
    x.ok(efe_down_adam_step(x.c, P(grad), x.state(exp_avg, "exp_avg", NP), x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
}

// the same two at every admitted geometry (csrc/train_down_g.hip behind k_adam_down): the flat vectors have efe_param_count("down_g") elements
std::vector<Tensor> train_down_g(int64_t h, const Tensor& o1_, const Tensor& pm_, const Tensor& pv_, double gamma, double beta_s, double beta_o, int64_t omega_mode,
                                 const OptT& omega, double omega_scalar, int64_t seed, int64_t stage, int64_t pass, int64_t sample, int64_t row_offset,
                                 const OptT& eps, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double aeps, int64_t step) {
    Ctx x(h);
    const int64_t NP = x.param_count("down_g");
    DownIn in = down_in(x, o1_, pm_, pv_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, seed, stage, pass, sample, row_offset, eps);
    auto op = in.o1.options();
    const int64_t M = in.M;
    Tensor F = at::empty({M}, op), nl = at::empty({M}, op), kls = at::empty({M}, op), kln = at::empty({M}, op);
    efe_fe_out out{};
    out.F_down = P(F); out.nlogpo1 = P(nl); out.kl_s = P(kls); out.kl_naive = P(kln);
    const efe_adam_params hp = adam_params(lr, beta1, beta2, aeps, step);
    x.ok(efe_train_down_g(x.c, P(in.o1), P(in.pm), P(in.pv), in.M, &in.p, &in.nz, in.eps, &out, x.state(exp_avg, "exp_avg", NP),
                          x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
    return {F, nl, kls, kln};
}

void down_adam_step_g(int64_t h, const Tensor& grad_, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step) {
    Ctx x(h);
    const int64_t NP = x.param_count("down_g");
    Tensor grad = x.f32(grad_, "grad");
    TORCH_CHECK(grad.numel() == NP, "efe: grad has ", grad.numel(), " elements, ModelDown has ", NP, " parameters");
    const efe_adam_params hp = adam_params(lr, beta1, beta2, eps, step);
    x.ok(efe_down_adam_step_g(x.c, P(grad), x.state(exp_avg, "exp_avg", NP), x.state(exp_avg_sq, "exp_avg_sq", NP), &hp, x.stream()));
}

// one whole training step, train.py:111-126 (efe_train_step) -> (kl_pi, omega, qs0, F_mid, ps1_mean, ps1_logvar, F_down, nlogpo1, kl_s, kl_naive); means
// [EFE_STEP_MEANS] and the six state vectors are written in place.  hyper = (lr, beta1, beta2, eps) of the top, mid and down optimisers
// (12 numbers), steps = their three step numbers
std::vector<Tensor> train_step(int64_t h, const Tensor& o0_, const Tensor& o1_, const Tensor& pi0_, const Tensor& lp_, double gamma, double beta_s,
                               double beta_o, int64_t omega_mode, const OptT& omega, double omega_scalar, double a, double b, double cc, double d,
                               int64_t seed, int64_t stage, int64_t row_offset, const OptT& eps, Tensor top_m, Tensor top_v, Tensor mid_m, Tensor mid_v,
                               Tensor down_m, Tensor down_v, c10::ArrayRef<double> hyper, at::IntArrayRef steps, Tensor means) {
    Ctx x(h);
    TORCH_CHECK(x.C == 1 && x.R == 64, "efe engine: efe_train_step: built for the 1 x 64 x 64 geometry only");
    TORCH_CHECK(hyper.size() == 12 && steps.size() == 3, "efe: train_step takes 12 hyper-parameters and 3 step numbers");
    StepIn in = step_in(x, o0_, o1_, pi0_, lp_, gamma, beta_s, beta_o, omega_mode, omega, omega_scalar, a, b, cc, d, seed, stage, row_offset, eps);
    const int64_t Pt = x.param_count("top"), Pm = x.param_count("ps_net"), Pd = x.param_count("down");
    efe_step_adam at_{x.state(top_m, "top exp_avg", Pt), x.state(top_v, "top exp_avg_sq", Pt), adam_params(hyper[0], hyper[1], hyper[2], hyper[3], steps[0])};
    efe_step_adam am_{x.state(mid_m, "mid exp_avg", Pm), x.state(mid_v, "mid exp_avg_sq", Pm), adam_params(hyper[4], hyper[5], hyper[6], hyper[7], steps[1])};
    efe_step_adam ad_{x.state(down_m, "down exp_avg", Pd), x.state(down_v, "down exp_avg_sq", Pd), adam_params(hyper[8], hyper[9], hyper[10], hyper[11], steps[2])};
    auto op = in.o0.options();
    const int64_t M = in.M, S = x.s;
    std::vector<Tensor> r = {at::empty({M}, op), at::empty({M}, op), at::empty({M, S}, op), at::empty({M}, op), at::empty({M, S}, op),
                             at::empty({M, S}, op), at::empty({M}, op), at::empty({M}, op), at::empty({M}, op), at::empty({M}, op)};
    efe_step_in si{P(in.o0), P(in.o1), P(in.pi0), P(in.lp), in.eps};
    efe_step_out out{P(r[0]), P(r[1]), P(r[2]), P(r[3]), P(r[4]), P(r[5]), P(r[6]), P(r[7]), P(r[8]), P(r[9]), x.state(means, "means", EFE_STEP_MEANS)};
    x.ok(efe_train_step(x.c, &si, in.M, &in.p, &in.nz, &at_, &am_, &ad_, &out, x.stream()));
    return r;
}

// the epoch report, train.py:136-187 (efe_eval_stats): batch statistics of an evaluation batch into out [EFE_EVAL_STATS], written in place.
// A group is given whole or not at all; the engine refuses anything else (and M outside [1, EFE_EVAL_MAX_ROWS]) before it launches, so
// the sizes are checked here only where the engine would go on to read them.
void eval_stats(int64_t h, const OptT& F_top, const OptT& F_mid, const OptT& F_down, const OptT& nlogpo1, const OptT& kl_s, const OptT& kl_naive,
                const OptT& kl_pi, const OptT& kl_s_anal, const OptT& kl_naive_anal, const OptT& kl_pi_anal, const OptT& qs1, const OptT& s0,
                const OptT& S_real, const OptT& o1_r, const OptT& po1_r, int64_t M, int64_t Mr, Tensor out) {
    Ctx x(h);
    TORCH_CHECK(M >= INT32_MIN && M <= INT32_MAX && Mr >= INT32_MIN && Mr <= INT32_MAX, "efe engine: efe_eval_stats: M / Mr out of range");
    const bool sized = M >= 1 && M <= EFE_EVAL_MAX_ROWS, rsized = Mr >= 1 && Mr <= EFE_EVAL_MAX_ROWS;
    Tensor keep[15];
    auto arg = [&](const OptT& t, int slot, const char* name, int64_t rows_, int64_t width, bool check) -> const float* {
        if (!given(t)) return nullptr;
        keep[slot] = x.f32(*t, name);
        TORCH_CHECK(!check || keep[slot].numel() == rows_ * width, "efe engine: efe_eval_stats: ", name, " has ", keep[slot].numel(), " elements, expected ",
                    rows_, " x ", width);
        return P(keep[slot]);
    };
    efe_eval_in ei{};
    ei.F_top = arg(F_top, 0, "F_top", M, 1, sized); ei.F_mid = arg(F_mid, 1, "F_mid", M, 1, sized); ei.F_down = arg(F_down, 2, "F_down", M, 1, sized);
    ei.nlogpo1 = arg(nlogpo1, 3, "nlogpo1", M, 1, sized); ei.kl_s = arg(kl_s, 4, "kl_s", M, 1, sized); ei.kl_naive = arg(kl_naive, 5, "kl_naive", M, 1, sized);
    ei.kl_pi = arg(kl_pi, 6, "kl_pi", M, 1, sized); ei.kl_s_anal = arg(kl_s_anal, 7, "kl_s_anal", M, x.s, sized);
    ei.kl_naive_anal = arg(kl_naive_anal, 8, "kl_naive_anal", M, x.s, sized); ei.kl_pi_anal = arg(kl_pi_anal, 9, "kl_pi_anal", M, x.A, sized);
    ei.qs1 = arg(qs1, 10, "qs1", M, x.s, sized); ei.s0 = arg(s0, 11, "s0", M, x.s, sized); ei.S_real = arg(S_real, 12, "S_real", M, 6, sized);
    ei.o1_r = arg(o1_r, 13, "o1_r", Mr, 4096, rsized); ei.po1_r = arg(po1_r, 14, "po1_r", Mr, 4096, rsized);
    ei.Mr = (int)Mr;
    x.ok(efe_eval_stats(x.c, &ei, (int)M, x.state(out, "out", EFE_EVAL_STATS), x.stream()));
}

// the mutual information of every latent with every true factor (efe_eval_mi) into out [EFE_EVAL_MI], written in place; noise: float64
// [EFE_EVAL_MI, 2, M] or none (device noise from seed and stage); counts: int32 [EFE_EVAL_MI, 2, M] or none.  The engine refuses
// n_neighbors and M out of range before it launches, so the sizes are checked here only where it would go on to read them.
void eval_mi(int64_t h, const Tensor& s0_, const Tensor& S_real_, const OptT& noise, int64_t n_neighbors, int64_t seed, int64_t stage, Tensor out,
             const OptT& counts) {
    Ctx x(h);
    Tensor s0 = x.f32(s0_, "s0"), S = x.f32(S_real_, "S_real"), nk;
    const int64_t M = s0.dim() ? s0.size(0) : 1;
    TORCH_CHECK(M <= INT32_MAX && n_neighbors >= INT32_MIN && n_neighbors <= INT32_MAX, "efe engine: efe_eval_mi: M / n_neighbors out of range");
    const bool sized = M >= 1 && M <= EFE_EVAL_MAX_ROWS;
    TORCH_CHECK(!sized || (s0.numel() == M * 10 && S.numel() == M * 6), "efe engine: efe_eval_mi: s0 / S_real have ", s0.numel(), " / ", S.numel(),
                " elements, expected ", M, " x 10 and ", M, " x 6");
    efe_eval_mi_in mi{};
    mi.s0 = P(s0); mi.S_real = P(S);
    if (given(noise)) {
        nk = x.check(*noise, "noise", at::kDouble).contiguous();
        TORCH_CHECK(!sized || nk.numel() == (int64_t)EFE_EVAL_MI * 2 * M, "efe engine: efe_eval_mi: noise has ", nk.numel(), " elements, expected 60 x 2 x ", M);
        mi.noise = nk.data_ptr<double>();
    }
    mi.n_neighbors = (int)n_neighbors; mi.seed = (uint64_t)seed; mi.stage = (uint32_t)stage;
    int32_t* cp = nullptr;
    if (given(counts)) {
        TORCH_CHECK(x.check(*counts, "counts", at::kInt).is_contiguous() && (!sized || counts->numel() == (int64_t)EFE_EVAL_MI * 2 * M),
                    "efe engine: efe_eval_mi: counts must be a contiguous int32 tensor of 60 x 2 x ", M, " elements");
        cp = counts->data_ptr<int32_t>();
    }
    x.ok(efe_eval_mi(x.c, &mi, (int)M, x.state(out, "out", EFE_EVAL_MI), cp, x.stream()));
}

}  // namespace

TORCH_LIBRARY(efe, m) {
    m.def("transition(int ctx, Tensor pi, Tensor s0, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor ps1, Tensor mean, Tensor logvar)");
    m.def("decoder(int ctx, Tensor s, int seed, int stage, int pass_id, int sample, int row_offset) -> Tensor");
    m.def("encoder(int ctx, Tensor o, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, bool want_s) -> (Tensor s, Tensor mean, Tensor logvar)");
    m.def("encoder_rows(int ctx, Tensor o, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, bool want_s, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor s, Tensor mean, Tensor logvar)");
    m.def("rollout_rows(int ctx, Tensor o, Tensor pi, int steps, int samples, bool calc_mean, bool per_stage_mean, int seed, int stage, int row_offset, Tensor? eps, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor sum_G, Tensor sum_terms, Tensor po1)");
    m.def("habit(int ctx, Tensor s) -> (Tensor logits, Tensor q, Tensor logq)");
    m.def("calculate_g(int ctx, Tensor s0, Tensor pi0, int samples, bool mean_mode, int seed, int stage, int row_offset, Tensor? eps, Tensor? mask=None, Tensor? ids=None, int rows_per_entry=1, int n_total=0) -> (Tensor G, Tensor terms, Tensor ps1, Tensor ps1_mean, Tensor po1, Tensor t2parts)");
    m.def("rollout(int ctx, Tensor o, Tensor pi, int steps, int samples, bool calc_mean, bool per_stage_mean, int seed, int stage, int row_offset, Tensor? eps) -> (Tensor sum_G, Tensor sum_terms, Tensor po1)");
    m.def("trajectory(int ctx, Tensor s0_traj, Tensor ps1_traj, Tensor ps1_mean_traj, Tensor ps1_logvar_traj, Tensor pi0_traj, int seed, int stage, int row_offset, Tensor? eps) -> Tensor");
    m.def("simulate(int ctx, Tensor starting_s, int depth, bool use_means, int seed, int stage, int row_offset, Tensor? eps, Tensor? u, Tensor? mask=None, Tensor? ids=None, int n_total=0) -> (Tensor G, Tensor pi0, Tensor Qpi0)");
    m.def("action_posterior(int ctx, Tensor sum_G, int n, float temperature) -> (Tensor P, Tensor logP)");
    m.def("check_reward(int ctx, Tensor o) -> Tensor");
    m.def("reparameterize(int ctx, Tensor mean, Tensor logvar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> Tensor");
    m.def("free_energy(int ctx, Tensor o0, Tensor o1, Tensor pi0, Tensor log_Ppi, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, float a, float b, float c, float d, int seed, int stage, int row_offset, Tensor? eps) -> Tensor[]");
    m.def("loss_top(int ctx, Tensor s, Tensor log_Ppi) -> (Tensor F_top, Tensor kl_pi, Tensor kl_pi_anal, Tensor Qpi)");
    m.def("loss_mid(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor F_mid, Tensor kl_s, Tensor kl_s_anal, Tensor ps1, Tensor ps1_mean, Tensor ps1_logvar)");
    m.def("loss_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> (Tensor F_down, Tensor nlogpo1, Tensor kl_s, Tensor kl_s_anal, Tensor kl_naive, Tensor kl_naive_anal, Tensor po1, Tensor qs1)");
    m.def("top_grad(int ctx, Tensor s, Tensor log_Ppi) -> (Tensor kl_pi, Tensor grad)");
    m.def("adam_step(int ctx, str part, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> ()");
    m.def("train_top(int ctx, Tensor s, Tensor log_Ppi, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> Tensor");
    m.def("mid_grad(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset) -> (Tensor F_mid, Tensor ps1_mean, Tensor ps1_logvar, Tensor grad)");
    m.def("train_mid(int ctx, Tensor s0, Tensor Ppi_sampled, Tensor qs1_mean, Tensor qs1_logvar, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> (Tensor ps1_mean, Tensor ps1_logvar, Tensor F_mid)");
    m.def("dec_tail_grad(int ctx, Tensor h4, Tensor o1, float scale, float beta_o, bool want_y) -> (Tensor nlogpo1, Tensor po1, Tensor d_h4, Tensor grad, Tensor y1, Tensor y2, Tensor y3)");
    m.def("dec_grad(int ctx, Tensor s, Tensor o1, float scale, float beta_o, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]");
    m.def("enc_grad(int ctx, Tensor o, Tensor d_mean, Tensor d_logvar, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]");
    m.def("down_grad(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> Tensor[]");
    m.def("train_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float adam_eps, int step) -> Tensor[]");
    m.def("train_step(int ctx, Tensor o0, Tensor o1, Tensor pi0, Tensor log_Ppi, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, float a, float b, float c, float d, int seed, int stage, int row_offset, Tensor? eps, Tensor(a!) top_exp_avg, Tensor(b!) top_exp_avg_sq, Tensor(c!) mid_exp_avg, Tensor(d!) mid_exp_avg_sq, Tensor(e!) down_exp_avg, Tensor(f!) down_exp_avg_sq, float[] hyper, int[] steps, Tensor(g!) means) -> Tensor[]");
    m.def("eval_stats(int ctx, Tensor? F_top, Tensor? F_mid, Tensor? F_down, Tensor? nlogpo1, Tensor? kl_s, Tensor? kl_naive, Tensor? kl_pi, Tensor? kl_s_anal, Tensor? kl_naive_anal, Tensor? kl_pi_anal, Tensor? qs1, Tensor? s0, Tensor? S_real, Tensor? o1_r, Tensor? po1_r, int M, int Mr, Tensor(a!) out) -> ()");
    m.def("down_adam_step(int ctx, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> ()");
    m.def("eval_mi(int ctx, Tensor s0, Tensor S_real, Tensor? noise, int n_neighbors, int seed, int stage, Tensor(a!) out, Tensor(b!)? counts) -> ()");
}

TORCH_LIBRARY_IMPL(efe, CUDA, m) {       // the CUDA dispatch key is the HIP device on ROCm builds of PyTorch
    m.impl("transition", &transition);
    m.impl("decoder", &decoder);
    m.impl("encoder", &encoder);
    m.impl("encoder_rows", &encoder_rows);
    m.impl("rollout_rows", &rollout_rows);
    m.impl("habit", &habit);
    m.impl("calculate_g", &calculate_g);
    m.impl("rollout", &rollout);
    m.impl("trajectory", &trajectory);
    m.impl("simulate", &simulate);
    m.impl("action_posterior", &action_posterior);
    m.impl("check_reward", &check_reward);
    m.impl("reparameterize", &reparameterize);
    m.impl("free_energy", &free_energy);
    m.impl("loss_top", &loss_top);
    m.impl("loss_mid", &loss_mid);
    m.impl("loss_down", &loss_down);
    m.impl("top_grad", &top_grad);
    m.impl("adam_step", &adam_step);
    m.impl("train_top", &train_top);
    m.impl("mid_grad", &mid_grad);
    m.impl("train_mid", &train_mid);
    m.impl("dec_tail_grad", &dec_tail_grad);
    m.impl("dec_grad", &dec_grad);
    m.impl("enc_grad", &enc_grad);
    m.impl("down_grad", &down_grad);
    m.impl("train_down", &train_down);
    m.impl("train_step", &train_step);
    m.impl("eval_stats", &eval_stats);
    m.impl("down_adam_step", &down_adam_step);
    m.impl("eval_mi", &eval_mi);
}

// torch.ops.efe_g.* : the entry points that take their geometry from the context.  A namespace of its own: the 31 schemas of torch.ops.efe
// are pinned as a closed set (tests/test_abi.py), and these calls are additions beside them, not changes to them.
TORCH_LIBRARY(efe_g, m) {
    m.def("dec_tail_grad(int ctx, Tensor h4, Tensor o1, float scale, float beta_o, bool want_y) -> (Tensor nlogpo1, Tensor po1, Tensor d_h4, Tensor grad, Tensor y1, Tensor y2, Tensor y3)");
    m.def("dec_grad(int ctx, Tensor s, Tensor o1, float scale, float beta_o, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]");
    m.def("enc_grad(int ctx, Tensor o, Tensor d_mean, Tensor d_logvar, int seed, int stage, int pass_id, int sample, int row_offset, bool want_act) -> Tensor[]");
    m.def("down_grad(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps) -> Tensor[]");
    m.def("train_down(int ctx, Tensor o1, Tensor ps1_mean, Tensor ps1_logvar, float gamma, float beta_s, float beta_o, int omega_mode, Tensor? omega, float omega_scalar, int seed, int stage, int pass_id, int sample, int row_offset, Tensor? eps, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float adam_eps, int step) -> Tensor[]");
    m.def("down_adam_step(int ctx, Tensor grad, Tensor(a!) exp_avg, Tensor(b!) exp_avg_sq, float lr, float beta1, float beta2, float eps, int step) -> ()");
}

TORCH_LIBRARY_IMPL(efe_g, CUDA, m) {
    m.impl("dec_tail_grad", &dec_tail_grad_g);
    m.impl("dec_grad", &dec_grad_g);
    m.impl("enc_grad", &enc_grad_g);
    m.impl("down_grad", &down_grad_g);
    m.impl("train_down", &train_down_g);
    m.impl("down_adam_step", &down_adam_step_g);
}
