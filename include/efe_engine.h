/* efe_engine.h -- C ABI of the MI355X expected-free-energy (EFE) rollout engine.
 *
 * Drop-in boundary for the Monte-Carlo EFE hot path of zfountas/deep-active-inference-mc.
 * The reference has no FFI: its boundary is the Python object `ActiveInferenceModel`
 * (/root/reference/src/torchmodel.py:149-393).  Each entry point below replaces one method of that
 * object (cited per function); the Python mirror in deep-active-inference-mc_amd/model.py binds
 * them with ctypes and keeps the reference's method names, argument meaning and return tuples.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All tensor pointers are DEVICE pointers to
 *     contiguous fp32 unless the name ends in _host.  Observations are NCHW [M,1,64,64].
 *   - no ownership transfer: the caller allocates every input/output buffer; the engine owns only
 *     its packed weights and a scratch arena.  Calls are stream-ordered on `stream` (a hipStream_t
 *     passed as void*; NULL = default stream) and return without synchronising, unless the arena must
 *     grow (first call at a new size; efe_reserve pre-sizes it so that steady-state calls never hipMalloc).
 *   - threading / streams: a context has ONE scratch arena.  Every entry point, the getters and
 *     efe_last_call_macs included, first checks its handle against the library's registry of live
 *     contexts and takes the context's mutex, so several host threads may share a context (their calls
 *     serialise).  efe_destroy may be called while other threads are in calls on the same context: it
 *     waits for the call in progress, and calls admitted after it are refused (return code 1).  A call
 *     issued on a different stream than the previous call first waits (hipStreamWaitEvent) for that
 *     call's last kernel, so switching streams is safe and costs one event wait.  For concurrent
 *     execution on several streams use one context per stream (weights are 21 MB).
 *   - return value: 0 on success, non-zero on error (efe_last_error() gives the message).
 *   - noise: MC-dropout masks / normals / action uniforms are a pure function of
 *     (seed, stage, pass, sample, global row = row_offset + r, element) -- see csrc/philox.h --
 *     so results are independent of batching and of the number of GPUs.  `stage` is the caller's
 *     call counter: one calculate_G call (or one stage of a rollout) consumes one stage value.
 *     `eps` pointers are optional injected normals (NULL = generated on device).
 */
#ifndef EFE_ENGINE_H
#define EFE_ENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct efe_ctx efe_ctx;

/* lifecycle ------------------------------------------------------------------------------------ */
int efe_create(efe_ctx** out, int device);                       /* ActiveInferenceModel.__init__, torchmodel.py:150-165 (10, 4, 1, 64) */
/* ActiveInferenceModel(s_dim, pi_dim, ..., colour_channels, resolution), torchmodel.py:150: s_dim must be 10 (the reference never uses
 * another), pi_dim 2..6, channels 1..3, resolution a multiple of 4 in [32, 128].  (1, 64) is the Dynamic-dSprites geometry on the fused
 * kernels; any other geometry (BASELINE configs[4]: pi 3, 3 x 84 x 84) is BUILD-DEFINED -- the reference rejects it (torchmodel.py:77-82)
 * and its reward (calc_reward_animalai, torchmodel.py:214) is undefined -- and runs the generic convolution path: encoder
 * Conv2d(k3,s2) x 4 + dense head with 64 * h4 * h4 inputs, decoder dense head -> Linear(256, 64 * (res/4)^2) -> ConvT(64,64,s1) ->
 * ConvT(64,64,s2) -> ConvT(64,32,s2) -> ConvT(32,C,s1) + sigmoid (resolution 32 = the reference's own variant, torchmodel.py:77-80: decoder base
 * 16 x 16 and a stride-1 third layer; its NETWORKS are pinned against the reference, tests/golden/nets32_*.npz), reward = SUM over (c,h,w) of the NCHW-broadcast log-likelihood of
 * torchutils.py:34-37.  Observations are NCHW [M, C, res, res].  Parity unpinned: validated against oracle/efe_oracle.py (cfg=) only. */
int efe_create_cfg(efe_ctx** out, int device, int s_dim, int pi_dim, int channels, int resolution);
int efe_get_config(efe_ctx* ctx, int* s_dim, int* pi_dim, int* channels, int* resolution);      /* outputs may be NULL */
/* the HIP device the context was created on (efe_create's `device`) and the PCI bus id string of that device ("0000:c1:00.0"; buf may be
 * NULL): what a multi-GPU launcher checks so that rank r really owns GPU r (bench.py gathers them and refuses two ranks on one device) */
int efe_get_device(efe_ctx* ctx, int* device, char* pci_bus_id, int pci_bus_id_len);
/* Removes the context from the registry, so that later calls with it are refused; waits for a call in progress on another thread; the
 * context's memory is released (after a device synchronisation) once no call holds it.  A handle that is not live (already destroyed,
 * never created) is ignored. */
void efe_destroy(efe_ctx* ctx);
const char* efe_last_error(efe_ctx* ctx);
/* 1 if `ctx` is a live context of this process (created by efe_create[_cfg], not yet destroyed), else 0; never dereferences the pointer.
 * The library keeps a registry of its contexts and EVERY entry point checks its handle against it first, before it reads the context: a
 * stale or made-up handle is return code 1 (efe_last_call_macs: 0, efe_rollout_scratch_bytes: 0) and efe_last_error reads "stale or
 * invalid context handle", never a use of freed memory, also when efe_destroy runs on another thread.  Bindings that carry the handle as an
 * integer (torch.ops.efe.*, ctypes) use this to raise a proper error.  Every entry point also restores the CALLER's current HIP device
 * before it returns (the context's device is current only inside the call). */
int efe_ctx_alive(const efe_ctx* ctx);
int efe_abi_version(void);                                       /* 6 (history of the versions: INTEGRATION.md section 4) */
/* hex digest of the sources this library was compiled from (build.py stamps it; the Python loader refuses a library whose
 * digest differs from the sources next to it, so a stale shipped binary fails loudly). */
const char* efe_build_id(void);

/* weights: reference state_dict tensors (host, reference layout), key = "<top|mid|down>.<state_dict key>",
 * e.g. "down.po_net.13.weight" (ConvTranspose2d [Cin,Cout,3,3]).  Replaces load_weights,
 * torchmodel.py:173-177 (the .pth unpickling stays in Python).  efe_commit_weights packs them into the
 * MFMA fragment-major device layout.  The host copies are kept: after a commit a caller may update any subset of
 * tensors with efe_set_weight and commit again; the packed buffers of the previous commit are freed (no growth). */
int efe_set_weight(efe_ctx* ctx, const char* key, const float* data_host, const int64_t* shape, int ndim);
int efe_commit_weights(efe_ctx* ctx);

/* options
 *   launch groups : "dec_chunk" (decoder rows per launch group), "enc_chunk", "dec_chunk_g" / "dec_budget_g" (generic-geometry decoder: cap in
 *                   images / in bytes of layer activations per launch group; 0.68 MB per image at 84 x 84, default budget 28 GiB)
 *   semantics     : "reward_upstream_intent" (0 / 1, default 0).  0 = the reward the shipped port computes (torchutils.py:34-37 on NCHW input: target
 *                   1 for image rows h < H/2, every pixel counts; pinned by the oracle).  1 = what the upstream NHWC code means:
 *                   only the top three rows count, target 1 on their left half; dSprites: mean over those 192 pixels * 10, other geometries: sum.
 *   A / B         : "fuse_final_g" (generic path: last two decoder layers in one kernel, default 1), "sim_split" (efe_simulate of <= 16 episodes: the habit-policy chain on eight workgroups per 8 episodes that split
 *                   the two wide transition layers, default 1, bit-identical to 0), "enc_tiled" (generic path, encoder layers 1 and 2: 2 = one
 *                   kernel with conv1 kept in LDS (default), 1 = LDS-tiled, one launch per layer, 0 = the direct kernel for every layer; bit-identical),
 *                   "ct_fuse12" (generic path: the decoder's first two ConvTranspose layers in one kernel, layer 1's output kept in LDS, default 1,
 *                   bit-identical to 0), "mid_unfused" (layer-by-layer transition MLP), "head_unfused" (the decoder / encoder dense heads as
 *                   one k_dense launch per layer instead of one k_head launch per head; same masks, fp32 summation order differs),
 *                   "dec_fuse_ab" (Dynamic dSprites, fp32 decoder launches of > 128 images: 1 = the two decoder tail kernels as one persistent
 *                   launch whose workgroups keep the activation between them in a 256 KiB slot each, 128 MiB of scratch instead of 256 KiB per
 *                   image of a launch group (default); 0 = two launches; bit-identical.  While efe_prof_enable times either decoder tail class
 *                   the call runs the two launches: one launch has no boundary between the classes), "dec_ab_grid" (cap of that launch's grid,
 *                   0 = min(512, images): lets a small launch give every workgroup several images; tests).  None of them removes work:
 *                   every setting computes the same quantities (fp32 summation order may differ where stated).
 *   experiment    : "mfma_bf16x3" (0 / 1, default 0; Dynamic-dSprites geometry only).  1 = the decoder's Linear(256, 16384) and its first two
 *                   ConvTranspose layers run on the bf16 matrix pipe with both operands split into three bf16 planes (six products per fp32
 *                   product, fp32 accumulation: csrc/bf16x3.hip).  Inputs narrower than the reference's fp32 arithmetic, results inside the same
 *                   tolerances (every fixture is run through it); never the default, never the benchmark's headline.  With it, results are no
 *                   longer bit-identical across launch sizes (launches of <= 128 images keep the fp32 small-launch kernels), only within tolerance.
 *                   "mfma_f16x2" (0 / 1, default 0; same scope): the same layers with two fp16 planes (weights scaled by a power of two).  An
 *                   activation beyond fp16's range poisons its row / image, and the result is NaN, never a finite wrong number: the poison
 *                   only travels through the split kernels, so under this option launches of <= 128 images run all four layers on the
 *                   exact fp32 kernels and ConvT3 always runs split ("b3_convt3" = 0 applies to mfma_bf16x3 alone).
 *   development   : "poison" (pre-fill scratch with a byte), "trace" (synchronise and log every profiled launch), "arena_align", "check_rows"
 *                   (range-check efe_rows.ids against efe_rows.n_total on the host before every _rows call: one synchronisation per call) */
int efe_set_option(efe_ctx* ctx, const char* name, int64_t value);

/* scratch arena: efe_reserve makes the arena one block of >= bytes (synchronises once); efe_rollout_scratch_bytes is the exact
 * arena use of efe_rollout(M, steps, samples) with the current options (sum_terms == NULL; 3 M floats less, rounded up to the
 * arena's alignment, with a sum_terms output) plus 1 MiB of head-room.  efe_rollout can run at one sample per stage (calc_mean &&
 * per_stage_mean): the returned value is then an upper bound.  efe_arena_stats reports capacity, the largest use of any call so
 * far and how many hipMalloc calls the arena has made (outputs may be NULL). */
int efe_reserve(efe_ctx* ctx, int64_t bytes);
int64_t efe_rollout_scratch_bytes(efe_ctx* ctx, int M, int steps, int samples);
int efe_arena_stats(efe_ctx* ctx, int64_t* capacity_bytes, int64_t* high_water_bytes, int64_t* grow_count);

/* The row set of ONE efe_calculate_g_rows / efe_simulate_rows call (ABI 4) -- the lock-step planner's early-stopped episodes (the
 * per-episode break of /root/reference/src/mcts.py:176).  The rows of a call are grouped into ENTRIES of rows_per_entry consecutive rows
 * (efe_calculate_g_rows: the pi_dim action rows of an episode; efe_simulate_rows: one episode = one entry, rows_per_entry ignored).
 *   mask : DEVICE array, one byte per entry ID, read when the kernels run (earlier work on the same stream may update it); the per-image
 *          kernels (decoder stages, encoder trunk: ~90 % of the work) skip dead entries, whose outputs are then unspecified; live rows
 *          are bit-identical to an unmasked call.  NULL = all live.
 *   ids  : DEVICE array, entry slot -> entry ID: the call's entry i IS entry ids[i] of the un-compacted batch -- its noise keys are those of
 *          rows ids[i] * rows_per_entry + k (plus efe_noise.row_offset) and the mask is read at ids[i].  A planner that has lost episodes
 *          passes only the live ones (a dense, smaller call) and still draws exactly what the full batch would.  NULL = identity.
 *   n_total : entries of the UN-COMPACTED batch = the length of `mask` and the exclusive upper bound of every id (ABI 5).  0 = not stated.
 *          When stated, a call with more entries than n_total (no ids) fails, and with the development option "check_rows" = 1 the
 *          ids are copied back and range-checked before the launch (one synchronisation: a stale or corrupt id would otherwise be a
 *          silent out-of-bounds read of `mask` and a wrong noise key).
 * A NULL efe_rows* means "all rows, identity" (the context-state shim efe_set_row_mask of ABI 2 - 5 is gone in ABI 6: the row set is an argument). */
typedef struct efe_rows {
    const uint8_t* mask;
    const int32_t* ids;
    int32_t rows_per_entry;
    int32_t n_total;
} efe_rows;

typedef struct efe_noise {
    uint64_t seed;
    uint32_t stage;       /* call / stage counter */
    uint32_t pass;        /* network-level calls only: which pass id keys the masks (csrc/philox.h) */
    uint32_t sample;      /* network-level calls only */
    uint32_t row_offset;  /* global index of local row 0 */
} efe_noise;

/* network level ---------------------------------------------------------------------------------- */
/* ModelMid.transition_with_sample, torchmodel.py:58-66.  eps: optional [M,10]. */
int efe_transition(efe_ctx*, const float* pi /*[M,4]*/, const float* s0 /*[M,10]*/, int M, const efe_noise* nz,
                   const float* eps, float* ps1, float* mean, float* logvar, void* stream);
/* ModelDown.decoder, torchmodel.py:139-141.  po: [M,1,64,64]. */
int efe_decoder(efe_ctx*, const float* s /*[M,10]*/, int M, const efe_noise* nz, float* po, void* stream);
/* ModelDown.encoder / encoder_with_sample, torchmodel.py:134-137,143-146.  s may be NULL. */
int efe_encoder(efe_ctx*, const float* o /*[M,1,64,64]*/, int M, const efe_noise* nz, const float* eps,
                float* s, float* mean, float* logvar, void* stream);
/* the same over the row set `rows` (1 x 64 x 64 geometry only; entry = rows_per_entry consecutive rows): row r of the call draws the noise of
 * global row ids[r / rows_per_entry] * rows_per_entry + r % rows_per_entry (+ nz->row_offset) -- the dense head's dropout masks and the
 * sample's normals -- so a compacted call returns the bits the full call returns for those rows; the trunk skips dead entries of `mask`
 * (their outputs are unspecified).  o, eps and the outputs are in the call's (compact) row order.  rows == NULL: efe_encoder. */
int efe_encoder_rows(efe_ctx*, const float* o /*[M,1,64,64]*/, int M, const efe_noise* nz, const float* eps, const efe_rows* rows,
                     float* s, float* mean, float* logvar, void* stream);
/* ModelTop.encode_s, torchmodel.py:27-31 (no dropout). */
int efe_habit(efe_ctx*, const float* s /*[M,10]*/, int M, float* logits, float* q, float* logq, void* stream);

/* ActiveInferenceModel.check_reward, torchmodel.py:210-212 (resolution-64 branch). o: [M,1,64,64] -> out [M]. */
int efe_check_reward(efe_ctx*, const float* o, int M, float* out, void* stream);
/* Model{Mid,Down}.reparameterize, torchmodel.py:54-56 / 130-132: out = eps * exp(logvar/2) + mean, [M,n];
 * eps optional (NULL = Philox normals keyed by nz->pass / sample / stage / row_offset). */
int efe_reparameterize(efe_ctx*, const float* mean, const float* logvar, int M, int n, const efe_noise* nz, const float* eps,
                       float* out, void* stream);

/* EFE level -------------------------------------------------------------------------------------- */
/* calculate_G (torchmodel.py:270-300) when mean_mode == 0; calculate_G_mean (torchmodel.py:302-327)
 * when mean_mode == 1 (samples forced to 1).
 * eps: optional [3*samples, M, 10] = T1_0..T1_{S-1}, T2_0..T2_{S-1}, D2B_0..D2B_{S-1}.
 * outputs: G[M], terms[3,M], ps1[M,10] (last sample; NULL ok), ps1_mean[M,10], po1[M,1,64,64] (last sample; NULL ok),
 * t2parts[2,M] (term2_1, term2_2; NULL ok). */
int efe_calculate_g(efe_ctx*, const float* s0, const float* pi0, int M, int samples, int mean_mode,
                    const efe_noise* nz, const float* eps,
                    float* G, float* terms, float* ps1, float* ps1_mean, float* po1, float* t2parts, void* stream);
/* the same over the row set `rows` (Node.expand of the lock-step planner, /root/reference/src/mcts.py:64-86 for every live episode at
 * once): M rows = M / rows_per_entry entries; inputs, eps and outputs are in the call's (compact) row order.  rows == NULL: as above. */
int efe_calculate_g_rows(efe_ctx*, const float* s0, const float* pi0, int M, int samples, int mean_mode,
                         const efe_noise* nz, const float* eps, const efe_rows* rows,
                         float* G, float* terms, float* ps1, float* ps1_mean, float* po1, float* t2parts, void* stream);

/* calculate_G_repeated (torchmodel.py:227-245) when per_stage_mean == 0;
 * calculate_G_4_repeated (torchmodel.py:247-268) semantics when per_stage_mean == 1 (calc_mean then
 * switches every stage to calculate_G_mean).  One row = one "EFE rollout".
 * nz->stage = stage0; stage t uses stage0 + t; the root encode uses (stage0, PASS_ROOT).
 * eps: optional [M*10 (root)] followed by per stage [3*S, M, 10].
 * outputs: sum_G[M], sum_terms[3,M], po1[M,1,64,64] (NULL ok). */
int efe_rollout(efe_ctx*, const float* o, const float* pi, int M, int steps, int samples, int calc_mean,
                int per_stage_mean, const efe_noise* nz, const float* eps,
                float* sum_G, float* sum_terms, float* po1, void* stream);

/* the same over the row set `rows` (1 x 64 x 64 geometry only): every draw of the call -- the root encoder's dropout, the root
 * reparameterisation and every stage of the core -- is keyed by the entry id as in efe_calculate_g_rows, so the rollouts of a compacted
 * subset (the games that decide on this tick, rows_per_entry = 4) are bit-identical to those rows of the full call; dead entries of `mask`
 * are skipped by the per-image kernels (outputs unspecified).  o, pi, eps and the outputs are in the call's row order.  rows == NULL:
 * efe_rollout. */
int efe_rollout_rows(efe_ctx*, const float* o, const float* pi, int M, int steps, int samples, int calc_mean,
                     int per_stage_mean, const efe_noise* nz, const float* eps, const efe_rows* rows,
                     float* sum_G, float* sum_terms, float* po1, void* stream);

/* calculate_G_given_trajectory (torchmodel.py:329-352): rows are trajectory steps. G[T]. */
int efe_trajectory(efe_ctx*, const float* s0_traj, const float* ps1_traj, const float* ps1_mean_traj,
                   const float* ps1_logvar_traj, const float* pi0_traj, int T, const efe_noise* nz, const float* eps,
                   float* G, void* stream);

/* mcts_step_simulate (torchmodel.py:354-393) for E lock-step episodes: habit-policy rollout of `depth`
 * steps from starting_s[E,10], then G over each trajectory.  Noise rows: steps use global row
 * row_offset+e (sample = t); trajectory rows use (row_offset+e)*depth + t.
 * eps: optional injected normals [depth][E][10] (the transition of step t) followed by [3][E*depth][10] (the trajectory's
 *      T1 slot (unused), T2, D2B -- the layout of efe_trajectory); u: optional injected action uniforms [depth][E].
 * outputs: G_mean[E], pi0[E,depth,4] one-hot, Qpi0[E,4] (habit posterior of the first step). */
int efe_simulate(efe_ctx*, const float* starting_s, int E, int depth, int use_means, const efe_noise* nz,
                 const float* eps, const float* u, float* G_mean, float* pi0, float* Qpi0, void* stream);
/* the same over the row set `rows` (entry = episode): episode slot e draws the noise of episode ids[e]; rows == NULL: as above. */
int efe_simulate_rows(efe_ctx*, const float* starting_s, int E, int depth, int use_means, const efe_noise* nz,
                      const float* eps, const float* u, const efe_rows* rows, float* G_mean, float* pi0, float* Qpi0, void* stream);

/* softmax_multi_with_log(-sum_G, n) (/root/reference/src/util.py:46-53,68): action posterior. */
int efe_action_posterior(efe_ctx*, const float* sum_G /*[n_groups*n]*/, int n_groups, int n, float temperature,
                         float* P, float* logP, void* stream);

/* Dynamic-dSprites environment, batched over E games (/root/reference/src/game_environment.py).
 * state [E,7] = (colour, shape, scale, orientation, x, y, accumulated reward), last_r [E]; all device pointers.
 * No engine weights are involved: these calls work on any context.
 *   efe_env_reset : randomize_environment_all (:72-75), latents / reward / last_r drawn from Philox(seed, stage).
 *   efe_env_new_image: new_image_all (:83-88): fresh latents from Philox(seed, stage); reward slot and last_r untouched
 *                   (what the reference constructor calls, :21).
 *   efe_env_step  : pi_to_action(actions[e], e, repeats) for every game (:113-169); a finished round resamples the
 *                   latents (new_image, :84-87) from Philox(seed, stage); round_changed [E] may be NULL.
 *   efe_env_render: s_to_o (:44-54): frames[e] = imgs[index(state[e])] (uint8 -> float, imgs is [n_imgs,64,64] uint8)
 *                   with the reward bar; err[e] = 1 where |last_r| > 1 (the reference raises ValueError), may be NULL. */
int efe_env_reset(efe_ctx*, float* state, float* last_r, int E, const efe_noise* nz, void* stream);
int efe_env_new_image(efe_ctx*, float* state, int E, const efe_noise* nz, void* stream);
int efe_env_step(efe_ctx*, float* state, float* last_r, const int32_t* actions, int E, int repeats, const efe_noise* nz,
                 int32_t* round_changed, void* stream);
int efe_env_render(efe_ctx*, const float* state, const float* last_r, const uint8_t* imgs, int64_t n_imgs, float* frames,
                   int32_t* err, int E, void* stream);

/* ---- per-game control state of the observe-plan-act loop (csrc/agent.hip; additive to ABI 6; /root/reference/test_demo.py:118-204) ------
 * All pointers are DEVICE arrays owned by the caller: queue [E][cap] int32 (test_demo.py's executing_steps; the queue of game g is
 * queue[g][head[g] .. head[g] + len[g])), head [E], len [E], crossings [E] (reward crossings so far) and reward_sum [E] (the rewards
 * received, added in tick order -- new_image restarts state slot 6 at 0 on every crossing, so the score the reference prints is not
 * the task reward).  Zero-filled arrays are the initial state; zeroing len (and head) clears every queue.  The kernels keep head == 0
 * whenever len == 0 and write a new queue from slot 0.  One thread per game; no engine weights are involved.
 *   efe_agent_need   : ids[0 .. *count) = the games whose queue is empty (:131), ASCENDING, *count (one device word) their number; a
 *                      function of `len` alone (no atomics).  ids has room for E entries; those at and beyond *count are not written.
 *   efe_agent_choose : the draw of :152-184 for the n deciding games ids[0 .. n): row i of the inputs belongs to game ids[i].
 *                      mode EFE_AGENT_AI : x = -(sum_G / steps)                             sum_G [4n]
 *                           EFE_AGENT_T1 : x = sum_terms[0] / steps                         sum_terms [3][4n]
 *                           EFE_AGENT_T12: x = sum_terms[0] / steps - sum_terms[1] / steps
 *                      p = exp(x / temperature) / sum, fp32, summed left to right, NO max-subtraction; EFE_AGENT_PROBS: p = probs [n][4].
 *                      The draw is np.random.choice's: cdf = cumsum(p) / cumsum(p)[3], the first edge above u; at u == 1.0 (which the
 *                      engine's 24-bit uniform can round to) the last action with p > 0.  u = u[i] when injected, else word 0 of the Philox
 *                      counter (tag 0x70, global game nz->row_offset + ids[i], stream 0, nz->stage); u_out [n] (NULL ok) receives it.
 *                      If any p is NaN, infinite or negative (exp overflow: inf / inf; all four underflow: 0 / 0) choice[i] = -1 and the
 *                      queue stays empty (the reference's `except: "Not executing anything"`): the game neither moves nor ticks this
 *                      tick and decides again on the next.  Otherwise the queue is choice[i] `repeat` times (steps * jumps for ai / t1 /
 *                      t12, steps for the habit method, :181-184).
 *   efe_agent_enqueue: queue of game ids[i] = actions[i][0 .. lengths[i]) (int32 [n][L], values 0..3; lengths clamped to [0, L]), each
 *                      action `jumps` times (the planner's path, :167-170).
 *   efe_agent_act    : one tick (:189-204).  A game with a non-empty queue takes its head action for exactly one tick of pi_to_action:
 *                      state, last_r and a crossing's new latents are bit-identical to efe_env_step(repeats = 1) at the same efe_noise
 *                      (seed, stage, row_offset = global index of game 0).  A crossing clears the queue, adds 1 to crossings and the
 *                      reward to reward_sum; otherwise the head advances.  A game with an empty queue is left untouched: no move, no
 *                      last_r *= 0.95.  round_changed [E] may be NULL.
 * Each call returns 1 with a message that names it, and launches nothing, for E < 1, n < 0 (or n > E), a cap smaller than the queue the
 * call would write, steps < 1, a temperature that is not finite and positive, an unknown mode, or a NULL required pointer. */
typedef struct efe_agent { int32_t* queue; int32_t* head; int32_t* len; int32_t* crossings; float* reward_sum; int32_t E, cap; } efe_agent;
typedef enum { EFE_AGENT_AI = 0, EFE_AGENT_T1 = 1, EFE_AGENT_T12 = 2, EFE_AGENT_PROBS = 3 } efe_agent_mode;
int efe_agent_need(efe_ctx*, const efe_agent* agent, int32_t* ids, int32_t* count, void* stream);
int efe_agent_choose(efe_ctx*, const efe_agent* agent, const int32_t* ids, int n, int mode, const float* sum_G, const float* sum_terms,
                     const float* probs, int steps, float temperature, int repeat, const efe_noise* nz, const float* u, int32_t* choice,
                     float* u_out, void* stream);
int efe_agent_enqueue(efe_ctx*, const efe_agent* agent, const int32_t* ids, int n, const int32_t* actions, const int32_t* lengths, int L,
                      int jumps, void* stream);
int efe_agent_act(efe_ctx*, const efe_agent* agent, float* state, float* last_r, const efe_noise* nz, int32_t* round_changed, void* stream);

/* ---- device-resident tree of the lock-step MCTS planner (counterpart of Node / active_inference_mcts, src/mcts.py:11-195) ----
 * All pointers are device pointers owned by the caller.  tree = { W, N, Qpi [E][cap][A] floats, child [E][cap][A] int32
 * (-1 = unexpanded), S [E][cap][s_dim] }.  One thread per episode; every formula in the reference's fp32 order with torch's
 * NaN rules (an unvisited edge makes Q = 0/0).  No engine weights are involved.
 *   efe_mcts_select  : tree policy (Node.select / probs_for_selection, :36-57) for every active episode: path_nodes / path_act
 *                      [E][max_depth], path_len [E], leaf [E], the leaf's state [E][s_dim] and its A-fold repeat [E*A][s_dim]
 *   efe_mcts_expand  : Node.expand bookkeeping (:64-86) where mask[e]: W[leaf] -= G, N[leaf] += 1, A children with states ps_next
 *   efe_mcts_backprop: Qpi[leaf] = q0, g = mean_r sims[r][e], W -= g and N += 1 along the path (:91-99, 186-191);
 *                      g_out [E] and active_out [E] are the iteration's history row
 *   efe_mcts_stop    : early stop (:130-131, 176) active[e] &= !(max(N0/sum) - mean(N0/sum) > threshold), stop_at[e] = repeat
 *                      for the episodes that stop now, *n_active = episodes still active */
typedef struct efe_mcts_tree { float* W; float* N; float* Qpi; int32_t* child; float* S; int32_t E, cap, A, s_dim; } efe_mcts_tree;
/* efe_mcts_step (ABI 4): the tree work between two iterations' engine calls as ONE launch, per episode in this order: efe_mcts_expand of the
 * PREVIOUS iteration's leaf (ABI 6: prev_n_nodes / prev_G / prev_ps_next, all three or none -- NULL: the caller has run efe_mcts_expand itself),
 * efe_mcts_backprop of the PREVIOUS iteration (prev_path_len == NULL: none; path_nodes / leaf must still hold that iteration's selection),
 * efe_mcts_stop, efe_mcts_select.  n_active: a zero-initialised word of its own per iteration (no memset is issued). */
int efe_mcts_step(efe_ctx*, const efe_mcts_tree* tree, const int32_t* prev_path_act, const int32_t* prev_path_len, const float* sims, int n_sims,
                  const float* q0, float* prev_g_out, uint8_t* prev_active_out, uint8_t* active, int32_t* stop_at, int repeat, float threshold,
                  int32_t* n_active, float C, int use_prior, int max_depth, int32_t* path_nodes, int32_t* path_act, int32_t* path_len, int32_t* leaf,
                  float* leaf_s, float* leaf_s_rep, int32_t* prev_n_nodes, const float* prev_G, const float* prev_ps_next, void* stream);
int efe_mcts_select(efe_ctx*, const efe_mcts_tree* tree, const uint8_t* active, float C, int use_prior, int max_depth,
                    int32_t* path_nodes, int32_t* path_act, int32_t* path_len, int32_t* leaf, float* leaf_s, float* leaf_s_rep,
                    void* stream);
int efe_mcts_expand(efe_ctx*, const efe_mcts_tree* tree, int32_t* n_nodes, const int32_t* nodes, const uint8_t* mask, const float* G,
                    const float* ps_next, void* stream);
int efe_mcts_backprop(efe_ctx*, const efe_mcts_tree* tree, const int32_t* path_nodes, const int32_t* path_act, const int32_t* path_len,
                      const int32_t* leaf, const uint8_t* active, const float* sims, int n_sims, const float* q0, int max_depth,
                      float* g_out, uint8_t* active_out, void* stream);
int efe_mcts_stop(efe_ctx*, const efe_mcts_tree* tree, uint8_t* active, int32_t* stop_at, int repeat, float threshold,
                  int32_t* n_active, void* stream);

/* ---- the two ends of an `mcts` decision of the agent loop (csrc/agent_mcts.hip; additive to ABI 6) ---------------------------------------
 * The n deciding games ids[0 .. n) (efe_agent_need) plan in the first n SLOTS of a planner's tree: every array below that is not part of
 * efe_agent is indexed by the slot i, the queue by the game ids[i].  One thread per slot, fp32, sums left to right.
 *   efe_agent_mcts_root   : the beginning of the decision (/root/reference/src/mcts.py:166-170).  Qpi [n][A] is the habit posterior of the root
 *                           state, A = 3 or 4; thr = max(Qpi) - mean(Qpi).
 *                             a Qpi row with a NaN, an infinite or a negative entry: choice[i] = -1, the queue stays empty, decided[i] = 1,
 *                               active[i] = 0 (efe_agent_choose's failure rule, whatever use_habit says);
 *                             use_habit != 0 and thr > threshold: choice[i] = a draw from Qpi by EFE_AGENT_PROBS's rule (cdf = cumsum / its
 *                               last entry, the first edge above u; u == 1.0: the last action with p > 0), the queue of game ids[i] becomes
 *                               that action `jumps` times (head 0), decided[i] = 1, active[i] = 0;
 *                             otherwise choice[i] = -2, the queue is not touched, decided[i] = 0, active[i] = 1: the planner goes on.
 *                           u = u[i] when injected, else word 0 of the Philox counter (tag 0x70, global game nz->row_offset + ids[i], stream 0,
 *                           nz->stage) -- the key of efe_agent_choose's uniform, so nz->stage is the tick; u_out [n] (NULL ok) receives it.
 *                           `active` is the planner's liveness mask (efe_mcts_step), `decided` is what efe_agent_mcts_enqueue skips.
 *   efe_agent_mcts_enqueue: the end (Node.action_selection, mcts.py:98-128, and test_demo.py:167-170).  For every slot with decided[i] == 0:
 *                           from node 0 of tree slot i, the argmax of N (NaN first, then the first index on ties) down to the first node
 *                           whose child[.][0] < 0; the visited actions trimmed as the reference trims them (a pair of opposite actions --
 *                           A = 4: 0/1 and 2/3, A = 3: 1/2 -- is dropped, and the last visited action is never emitted unless a pair consumed
 *                           it); the queue of game ids[i] becomes the trimmed path, each action `jumps` times, from slot 0 with head = 0.  A
 *                           path that trims to nothing leaves the queue empty: the game decides again on the next tick.  path_out
 *                           [n][max_depth] and path_len_out [n] (both NULL ok) receive the trimmed path; entries at and beyond the length
 *                           are not written.  Slots with decided[i] != 0 are not touched, in no array.  Of the tree only N, child, E (>= n),
 *                           cap and A are read.  The walk is cut after max_depth actions (the planner's is repeats + 2, above any depth its
 *                           tree can reach), so at most max_depth - 1 actions are queued.
 * Both return 1 with a message that names the call, and launch nothing, for E < 1, n outside [0, E], A other than 3 and 4, jumps < 1,
 * max_depth < 1, a queue capacity below max_depth * jumps (the longest queue the decision could write: refused where the decision begins,
 * not after the planning), or a NULL required pointer (root: neither nz nor u). */
int efe_agent_mcts_root(efe_ctx*, const efe_agent* agent, const int32_t* ids, int n, const float* Qpi /*[n][A]*/, int A, int use_habit,
                        float threshold, int max_depth, int jumps, const efe_noise* nz, const float* u, uint8_t* active, uint8_t* decided,
                        int32_t* choice, float* u_out, void* stream);
int efe_agent_mcts_enqueue(efe_ctx*, const efe_agent* agent, const efe_mcts_tree* tree, const int32_t* ids, int n, const uint8_t* decided,
                           int max_depth, int jumps, int32_t* path_out, int32_t* path_len_out, void* stream);

/* ---- the record of an agent run (csrc/agent_trace.hip; additive to ABI 6; what test_demo.py shows on every tick) -------------------------
 * efe_agent_trace is T rows (ticks) x E games of DEVICE arrays owned by the caller, row-major: state [T][E][7], last_r [T][E], action,
 * queue_len [T][E] int32, decided [T][E] uint8, choice [T][E] int32, u [T][E], G [T][E][4], terms [T][E][3][4], probs [T][E][4],
 * path [T][E][Lp] int32, path_len [T][E] int32.  The caller allocates them pre-filled with "nothing happened" (NaN for the floats, -1 for
 * action and choice, 0 for the rest): a call writes only what happened, nothing initialises a row.  None of these calls writes an array
 * of efe_agent or of the environment; no engine weights are involved.
 *   efe_agent_trace_tick    : row `row` of state / last_r = the environment now, action = the head of the queue (-1: the queue is empty
 *                             and efe_agent_act will not move the game), queue_len = its length.  Called after the tick's decision and
 *                             before its efe_agent_act.  (efe_agent_act's round_changed may point at a row of an [T][E] int32 array.)
 *   efe_agent_trace_decision: for the n deciding games ids[0 .. n) (inputs by slot i, the record by game ids[i]): decided = 1; choice and u
 *                             as given (NULL: the fill stays); mode EFE_AGENT_AI / T1 / T12: G = sum_G / steps, terms = (-sum_terms[0] /
 *                             steps, sum_terms[1] / steps, sum_terms[2] / steps) (test_demo.py:152-155, one fp32 division each; both
 *                             arrays are needed in all three modes) and probs = the p efe_agent_choose draws from in that mode, same bits;
 *                             EFE_AGENT_PROBS: probs = probs [n][4]; EFE_AGENT_NONE: no distribution.  path [n][path_stride] and
 *                             path_len [n] (both or neither): where path_len[i] >= 0, path_len is recorded as it is and the first
 *                             min(path_len[i], Lp, path_stride) actions of the path.
 *   efe_agent_plan_mask     : make_mask (test_demo.py:87-113) for the n deciding slots of an mcts decision into mask [E][32][32] at game
 *                             ids[i].  The explored paths of slot i are the history rows r < n_iter with H_active[r][i] != 0, cut to
 *                             H_len[r][i] (H_act [rows][h_slots][max_depth] int32, H_len [rows][h_slots] int32, H_active [rows][h_slots]
 *                             uint8).  The walker starts at (tx, ty) = (int(state[g][5]), int(state[g][4])) CLAMPED to 0..31 and takes
 *                             each action `jumps` times (0: tx + 1 if tx < 31, 1: tx - 1 if tx > 0, 2: ty + 1 if ty < 31, 3: ty - 1 if
 *                             ty > 0); a move that happens adds 1 to count[tx][ty]; mask = float(count) / float(max count), and ALL ZEROS
 *                             when nothing was counted (the reference divides 0 by 0).  Integer counters: independent of any order.
 *   efe_agent_view          : view [n][64][64] uint8 from frames [n][64][64] (efe_env_render): rows 59..62 of column 31 set to 1.0,
 *                             mask[ids[i]] (NULL: none) added onto rows and columns 16..47, then uint8(min(trunc(v * 255), 255)), NaN -> 0:
 *                             SATURATING where the reference's astype(uint8) wraps.
 * Each returns 1 with a message that names the call, and launches nothing, for E < 1, n outside [0, E], a row outside the record,
 * jumps < 1, A != 4 (mask), an unknown mode, or a NULL required pointer. */
typedef struct efe_agent_trace { float* state; float* last_r; int32_t* action; int32_t* queue_len; uint8_t* decided; int32_t* choice; float* u;
                                 float* G; float* terms; float* probs; int32_t* path; int32_t* path_len; int32_t T, E, Lp; } efe_agent_trace;
enum { EFE_AGENT_NONE = -1 };
int efe_agent_trace_tick(efe_ctx*, const efe_agent* agent, const efe_agent_trace* trace, int row, const float* state, const float* last_r,
                         void* stream);
int efe_agent_trace_decision(efe_ctx*, const efe_agent_trace* trace, int row, const int32_t* ids, int n, int mode, const int32_t* choice,
                             const float* u, const float* sum_G, const float* sum_terms, const float* probs, int steps, float temperature,
                             const int32_t* path, const int32_t* path_len, int path_stride, void* stream);
int efe_agent_plan_mask(efe_ctx*, const int32_t* ids, int n, int E, const float* state, const int32_t* H_act, const int32_t* H_len,
                        const uint8_t* H_active, int n_iter, int h_slots, int max_depth, int jumps, int A, float* mask, void* stream);
int efe_agent_view(efe_ctx*, const float* frames, const float* mask, const int32_t* ids, int n, int E, uint8_t* view, void* stream);


/* ---- training-side free energy, forward only (additive to ABI 6; /root/reference/src/torchloss.py, train.py:104-123) ----------------
 * efe_free_energy evaluates what one training step of train.py computes before its optimizer steps, for M rows:
 *   s0             = encoder_with_sample(o0)                                  pass PASS_FE_Q0 (9):   encoder masks + normals
 *   F_top, kl_pi, kl_pi_anal, Qpi = compute_loss_top(s0, log_Ppi)              (habit head, no noise)
 *   omega          = params->omega_mode: EFE_OMEGA_ARRAY (omega [M]), EFE_OMEGA_SCALAR (omega_scalar for every row), or
 *                    EFE_OMEGA_DERIVED: compute_omega(kl_pi, a, b, c, d) of this call (train.py's current_omega; defaults 1, 25, 5, 1.5)
 *   qs1_mean, qs1_logvar = encoder(o1)                                        pass PASS_FE_Q1 (10):  encoder masks
 *   F_mid, kl_s_mid, kl_s_mid_anal, ps1, ps1_mean, ps1_logvar = compute_loss_mid(s0, pi0, qs1_mean, qs1_logvar, omega)
 *                                                                              pass PASS_FE_T (11):   transition masks + normals
 *   F_down, nlogpo1, kl_s, kl_s_anal, kl_naive, kl_naive_anal, po1, qs1 = compute_loss_down(o1, ps1_mean, ps1_logvar, omega)
 *                                                                              pass PASS_FE_DOWN (12): encoder masks + normals, decoder masks
 * One stage (nz->stage) per call; nz->pass / nz->sample are not read (the four passes above, sample 0).  Rows are keyed by global row
 * nz->row_offset + r.  o0, o1: NCHW [M,C,H,W] fp32 (need not be binary); pi0 [M,pi_dim]; log_Ppi [M,pi_dim].
 * eps: NULL or injected normals [3][M][s_dim] = the FE_Q0, FE_T and FE_DOWN draws.
 * Every expression is the reference's in fp32 operation order (csrc/loss.hip); gamma is compared with 0.05 / 0.95 in fp32, as torch does
 * for its fp32 gamma tensor.  The BCE image sum has a fixed reduction order, so every output is bit-identical however the rows are
 * split over calls (with matching row_offset).  Under "mfma_bf16x3" / "mfma_f16x2" the decoder runs whatever the option selects, as in
 * efe_decoder, and F_down follows from that image.  A generic-geometry context works the same way (C*H*W pixels; parity unpinned). */
typedef enum { EFE_OMEGA_ARRAY = 0, EFE_OMEGA_SCALAR = 1, EFE_OMEGA_DERIVED = 2 } efe_omega_mode;
typedef struct efe_fe_params {
    float gamma, beta_s, beta_o;      /* ModelDown.gamma / beta_s / beta_o (the reference keeps them on ActiveInferenceModel, train.py:101) */
    int32_t omega_mode;               /* efe_omega_mode */
    const float* omega;               /* EFE_OMEGA_ARRAY: device [M] */
    float omega_scalar;               /* EFE_OMEGA_SCALAR */
    float a, b, c, d;                 /* EFE_OMEGA_DERIVED: compute_omega's parameters (train.py:29-32) */
} efe_fe_params;
/* outputs (device pointers; NULL = not wanted, except F_top / F_mid / F_down).  [M] unless stated; A = pi_dim, s = s_dim, image NCHW. */
typedef struct efe_fe_out {
    float* F_top; float* kl_pi; float* kl_pi_anal /*[M,A]*/; float* Qpi /*[M,A]*/;
    float* omega;
    float* F_mid; float* kl_s_mid; float* kl_s_mid_anal /*[M,s]*/; float* ps1 /*[M,s]*/; float* ps1_mean /*[M,s]*/; float* ps1_logvar /*[M,s]*/;
    float* F_down; float* nlogpo1 /* -sum log P(o1|s1) */; float* kl_s; float* kl_s_anal /*[M,s]*/; float* kl_naive; float* kl_naive_anal /*[M,s]*/;
    float* po1 /*[M,C,H,W]*/; float* qs1 /*[M,s]*/;
    float* s0 /*[M,s]*/; float* qs1_mean /*[M,s]*/; float* qs1_logvar /*[M,s]*/;
} efe_fe_out;
int efe_free_energy(efe_ctx*, const float* o0, const float* o1, const float* pi0, const float* log_Ppi, int M, const efe_fe_params* params,
                    const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream);
/* The three reference functions one by one, on the same kernels; noise follows the network-level convention (nz->pass / sample / stage /
 * row_offset key every mask and normal of the call), so loss_top(encoder_with_sample(o0, PASS_FE_Q0)), loss_mid(PASS_FE_T) and
 * loss_down(PASS_FE_DOWN) reproduce efe_free_energy bit for bit.  Only the outputs each function returns are read from `out`.
 *   efe_loss_top  : compute_loss_top(s [M,s], log_Ppi)                 -> F_top, kl_pi, kl_pi_anal, Qpi (no noise, nz unused)
 *   efe_loss_mid  : compute_loss_mid(s0, pi0, qs1_mean, qs1_logvar, omega) -> F_mid, kl_s_mid, kl_s_mid_anal, ps1, ps1_mean, ps1_logvar;
 *                   eps NULL or [M,s]
 *   efe_loss_down : compute_loss_down(o1, ps1_mean, ps1_logvar, omega)  -> F_down, nlogpo1, kl_s, kl_s_anal, kl_naive, kl_naive_anal,
 *                   po1, qs1 (+ qs1_mean / qs1_logvar of its own encoder pass); eps NULL or [M,s]
 * omega for loss_mid / loss_down: EFE_OMEGA_ARRAY or EFE_OMEGA_SCALAR (EFE_OMEGA_DERIVED needs kl_pi: efe_free_energy only). */
int efe_loss_top(efe_ctx*, const float* s, const float* log_Ppi, int M, efe_fe_out* out, void* stream);
int efe_loss_mid(efe_ctx*, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M,
                 const efe_fe_params* params, const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream);
int efe_loss_down(efe_ctx*, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, void* stream);

/* ---- training of the habit network (csrc/train.hip): train_model_top of /root/reference/src/torchloss.py:65-74 ----------------------------
 * One Adam step of ModelTop.qpi_net on F_top.mean(), F_top = sum_a Qpi (log(Qpi + 1e-20) - log_Ppi).  Its part name is "top".
 * The engine owns the weights (an fp32 master copy on the device next to the packed forward copies) and scratch; the gradient and the
 * optimiser state (exp_avg, exp_avg_sq) are DEVICE arrays of efe_param_count("top") floats owned by the caller, flat in the reference's
 * parameters() order (qpi_net.0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias), each row-major.  Every call is ordered on `stream`
 * like the other entry points: no synchronisation, no allocation in steady state.  Bad arguments and stale handles return 1.
 *   efe_top_grad   : s [M,s_dim], log_Ppi [M,pi_dim] -> kl_pi [M] (NULL: not wanted) and grad [P] = d mean(F_top) / d parameters.  The
 *                    gradient is a fixed-order sum: the same call twice gives the same bits.
 *   efe_adam_step  : torch.optim.Adam's default update (no amsgrad, no weight decay) of `part` with step number hp->step (1 for the first
 *                    step); writes the master copy and both packed forward copies, so every later call on the stream sees the new weights.
 *   efe_train_top  : both on the stream, bit-identical to efe_top_grad followed by efe_adam_step; kl_pi is that of the weights BEFORE
 *                    the update, as the reference returns it.
 *   efe_get_weights: the part's master copy -> dst (device, efe_param_count floats), ordered on the stream.
 * After a step the device copy is newer than the tensors given to efe_set_weight; efe_commit_weights and efe_set_weight("top....") first
 * bring those host copies up to date (one synchronisation), so a re-commit never reverts what was learnt. */
typedef struct efe_adam_params { double lr, beta1, beta2, eps; int64_t step; } efe_adam_params;
int64_t efe_param_count(efe_ctx*, const char* part);             /* 0: unknown part or stale handle */
int efe_get_weights(efe_ctx*, const char* part, float* dst, int64_t n, void* stream);
int efe_top_grad(efe_ctx*, const float* s, const float* log_Ppi, int M, float* kl_pi, float* grad, void* stream);
int efe_adam_step(efe_ctx*, const char* part, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream);
int efe_train_top(efe_ctx*, const float* s, const float* log_Ppi, int M, float* kl_pi, float* exp_avg, float* exp_avg_sq,
                  const efe_adam_params* hp, void* stream);

/* ---- training of the transition network (csrc/train.hip k_mid_grad): train_model_mid of the reference, src/torchloss.py:76-88 -----------
 * One Adam step of ModelMid.ps_net on F_mid.mean() (compute_loss_mid: the Gaussian KL of q(s1) against the transition's output with
 * precision omega).  The part's name is "ps_net", the reference's module name: efe_param_count, efe_get_weights and efe_adam_step take it
 * next to "top".  ("mid" is NOT a part name: a test of the habit-net commit pins it as refused, and existing tests do not change.)
 * P = efe_param_count("ps_net") = 543 252 at pi_dim 4, flat in parameters() order: ps_net.0.weight, 0.bias, 3.weight, 3.bias, 6.weight,
 * 6.bias, 9.weight, 9.bias.  Arguments follow efe_loss_mid: params->omega_mode EFE_OMEGA_ARRAY or EFE_OMEGA_SCALAR (EFE_OMEGA_DERIVED is
 * refused), nz keys the three MC-dropout masks (row nz->row_offset + r, pass, sample, stage); the reference's randn_like draw does not
 * enter the loss, so no normals are drawn.  ps1_mean / ps1_logvar [M,s_dim] and F_mid [M] are optional (NULL: not wanted); they agree
 * with efe_loss_mid's to rounding, not bit for bit (another summation order).
 *   efe_mid_grad  : -> grad [P] = d mean(F_mid) / d parameters, a fixed-order sum that depends on M alone: twice the same bits.
 *   efe_train_mid : efe_mid_grad and efe_adam_step("ps_net") on the stream, bit-identical to the two calls; the outputs are those of the
 *                   weights BEFORE the update, as the reference returns them.
 * Scratch (at most 8 partial gradients, 17 MB) comes from the context's arena.  efe_commit_weights and efe_set_weight("mid....") first
 * bring the host copies up to date, as for the habit net: re-committing any part never reverts a trained one. */
int efe_mid_grad(efe_ctx*, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                 const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* grad, void* stream);
int efe_train_mid(efe_ctx*, const float* s0, const float* pi0, const float* qs1_mean, const float* qs1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, float* ps1_mean, float* ps1_logvar, float* F_mid, float* exp_avg, float* exp_avg_sq,
                  const efe_adam_params* hp, void* stream);

/* ---- backward of the reconstruction loss through the decoder's ConvTranspose2d tail (csrc/train_dec.hip; additive to ABI 6) --------------
 * The first piece of train_model_down (src/torchloss.py:90-98): the four ConvTranspose2d layers po_net.13 / .15 / .17 / .19 with their
 * ReLUs, the sigmoid and the binary cross entropy of compute_loss_down (torchloss.py:62), at the 1 x 64 x 64 geometry.  No dropout lies
 * behind the Unflatten, so the call takes no noise keys.
 *   h4 [M,16384]   : what po_net[0:12] hands to the Unflatten, the reference's order (64, 16, 16) channel-major
 *   o1 [M,1,64,64] : the observed image
 *   scale, beta_o  : the loss is L = scale * sum_r nlogpo1_r.  scale >= 0 is used as given; a NEGATIVE scale means beta_o / M, the
 *                    decoder's share of F_down.mean() (gamma and beta_s touch only the KL terms, which do not reach po_net)
 *   nlogpo1 [M]    : -log p(o1), k_fe_down's expression and reduction order: bit-identical however rows are grouped (required)
 *   po1 [M,4096], d_h4 [M,16384] = dL / dh4 (no gate: the ReLU and dropout in front belong to the dense head), and the stored
 *   activations y1 [M,64,16,16], y2 [M,64,32,32], y3 [M,32,64,64] (NCHW, after the ReLU): optional, NULL = not wanted
 *   grad [P]       : dL / d parameters, P = efe_param_count("po_net_convt") = 92 609, flat in parameters() order (13.weight, 13.bias,
 *                    15.weight, 15.bias, 17.weight, 17.bias, 19.weight, 19.bias), each tensor row-major in the reference's shape (required)
 * A fixed-order sum that depends on M alone: twice the same bits; the per-row outputs do not depend on the other
 * rows of the call.  Scratch comes from the context's arena (rows are processed in groups of 64: at most 113 MB of activations and
 * gradients, and 32 partial gradients of 370 KB).  Returns 1 with a message that names the function for M <= 0, a NULL required pointer, a
 * context of another geometry, or a split-operand option (mfma_bf16x3 / mfma_f16x2) being on.  There is no optimiser step for this part
 * yet: efe_adam_step and efe_get_weights refuse the name. */
int efe_dec_tail_grad(efe_ctx*, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1, float* po1, float* d_h4,
                      float* grad, float* y1, float* y2, float* y3, void* stream);

/* ---- the same backward at every admitted geometry (csrc/train_dec_g.hip; additive to ABI 6) ------------------------------------------------
 * efe_dec_tail_grad's arguments and meaning with the sizes taken from the context (efe_create_cfg: C = 1..3 colour channels, resolution
 * R = 32..128 in steps of 4; B = R / 4, or 16 at R = 32, where the third layer has stride 1):
 *   h4, d_h4 [M, 64 B B]   o1, po1 [M,C,R,R]   y1 [M,64,B,B]   y2 [M,64,2B,2B]   y3 [M,32,R,R]   nlogpo1 [M]
 *   grad [P], P = efe_param_count("po_net_convt") = 92 320 + 289 C, parameters() order (19.weight is [32][C][3][3], 19.bias [C])
 * It runs kernels whose spatial sizes are run-time values at EVERY geometry, 1 x 64 x 64 included (there efe_dec_tail_grad's specialised
 * kernels are a cross-check: both hold the fp64 rule; their bits are not promised equal).  Same refusals (every one before the first launch),
 * same negative-scale rule, same per-row contract, same fixed-order sum (G = min(M, 32) slabs, row m in slab m mod G; DESIGN.md section
 * 7d-g): twice the same bits.  nlogpo1 is the 256-thread ordered sum over the row's C R R NCHW terms.  Rows are processed in groups of 64
 * (B <= 16) or 32 (B > 16): at most 231 MB of scratch activations and gradients at resolution 128, 99 MB at 3 x 84 x 84. */
int efe_dec_tail_grad_g(efe_ctx*, const float* h4, const float* o1, int M, float scale, float beta_o, float* nlogpo1, float* po1, float* d_h4,
                        float* grad, float* y1, float* y2, float* y3, void* stream);

/* ---- backward of the reconstruction loss through the whole decoder (csrc/train_dec_head.hip + csrc/train_dec.hip; additive to ABI 6) ------
 * The decoder's part of train_model_down (src/torchloss.py:90-98): po_net's dense head (Linear 10-256-256-256-16384, each with ReLU and
 * Dropout(0.5), torchmodel.py:107-118) evaluated for training, the ConvTranspose2d tail exactly as efe_dec_tail_grad runs it, and the
 * backward of both, at the 1 x 64 x 64 geometry.
 *   s [M,10]       : the decoder's input
 *   o1, scale, beta_o, nlogpo1, po1, y1..y3 : as efe_dec_tail_grad
 *   nz             : the keys of the four dropout masks: the FORWARD decoder's masks draw for draw (tag TAG_DEC + layer, global row
 *                    row_offset + r, stream_id(pass, sample), stage; the 16 384-feature mask keyed by the NHWC feature p 64 + c as in
 *                    efe_decoder), so efe_decoder with the same efe_noise decodes the same network: po1 agrees to rounding, not bit for
 *                    bit (another summation order).  The backward gate is read off the stored activation, 2 [h > 0].
 *   d_s [M,10] = dL / ds, and the stored activations after the mask h1, h2, h3 [M,256], h4 [M,16384] (the Unflatten's input, reference
 *   order c 256 + p): optional, NULL = not wanted
 *   grad [P]       : dL / d parameters, P = efe_param_count("po_net") = 4 437 697, flat in parameters() order (0.weight, 0.bias, 3.weight,
 *                    3.bias, 6.weight, 6.bias, 9.weight, 9.bias, then the tail's eight tensors exactly as efe_dec_tail_grad lays them out),
 *                    each tensor row-major in the reference's shape (required, as is nlogpo1)
 * A fixed-order sum that depends on M alone: twice the same bits; po1, nlogpo1, d_s, h1..h4 and y1..y3 of a row
 * depend on that row and its global row id only.  The tail's outputs are bit-identical to efe_dec_tail_grad on the returned h4.  Scratch
 * comes from the context's arena (rows are processed in groups of 64: the tail's scratch, plus at most 13 MB for the head and four
 * partial gradients of 538 KB).  Returns 1 with a message that names the function for M <= 0, a NULL required pointer, a context of
 * another geometry, or a split-operand option (mfma_bf16x3 / mfma_f16x2) being on.  There is no optimiser step for this part yet:
 * efe_adam_step and efe_get_weights refuse the name "po_net". */
int efe_dec_grad(efe_ctx*, const float* s, const float* o1, int M, float scale, float beta_o, const efe_noise* nz, float* nlogpo1, float* po1,
                 float* d_s, float* grad, float* h1, float* h2, float* h3, float* h4, float* y1, float* y2, float* y3, void* stream);

/* ---- the same whole-decoder backward at every admitted geometry (csrc/train_dec_head_g.hip + csrc/train_dec_g.hip; additive to ABI 6) ------
 * efe_dec_grad's arguments and meaning with the sizes taken from the context (C, R, B as efe_dec_tail_grad_g; F = 64 B B features of
 * po_net.9, 5 184 .. 65 536):
 *   s, d_s [M,10]   h1, h2, h3 [M,256]   h4 [M,F] (reference order c B B + p)   o1, po1 [M,C,R,R]   y1..y3 as efe_dec_tail_grad_g
 *   grad [P], P = efe_param_count("po_net") = 134 400 + 257 F + 92 320 + 289 C, parameters() order (9.weight is [F][256], 9.bias [F])
 * The masks are the forward decoder's at that geometry (efe_decoder; the F-feature mask keyed by the NHWC feature p 64 + c).  It runs
 * kernels whose feature count is a run-time value at EVERY geometry, 1 x 64 x 64 included (there efe_dec_grad is a cross-check: both hold
 * the fp64 rule; their bits are not promised equal).  Per row group it queues the head's forward, the tail exactly as efe_dec_tail_grad_g
 * runs it, and the head's backward: the tail's gradient, po1, nlogpo1 and y1..y3 are bit-identical to efe_dec_tail_grad_g on the returned
 * h4.  Same refusals as efe_dec_grad but the geometry's (every one before the first launch), same negative-scale rule, same per-row
 * contract; a fixed-order sum that depends on the geometry and M alone: twice the same bits.  Rows are processed
 * in groups of 64 (B <= 16) or 32: beside the tail's scratch at most 27 MB for the head (h4, d_h4 and the partial sums of d_h3, 8 MB each
 * at resolution 128) and four partial gradients of 538 KB.  There is no optimiser step for this part yet. */
int efe_dec_grad_g(efe_ctx*, const float* s, const float* o1, int M, float scale, float beta_o, const efe_noise* nz, float* nlogpo1, float* po1,
                   float* d_s, float* grad, float* h1, float* h2, float* h3, float* h4, float* y1, float* y2, float* y3, void* stream);

/* ---- gradient of F_down for all of ModelDown (csrc/train_enc.hip with the two decoder files; additive to ABI 6) --------------------------
 * train_model_down (src/torchloss.py:90-98) up to the gradient, at the 1 x 64 x 64 geometry: the encoder qs_net evaluated for training
 * (four stride-2 convolutions, Linear 576-256-256-256-20 with ReLU and Dropout(0.5) behind the first three, torchmodel.py:84-104, with
 * qs_net.9.weight [256][576]) and its backward, and the composed call that adds the sample, the decoder and the KL terms.
 * efe_param_count("qs_net") = 349 428 (0.weight, 0.bias, 2.*, 4.*, 6.*, 9.*, 12.*, 15.*, 18.*: parameters() order, each tensor row-major
 * in the reference's shape); efe_param_count("down") = 349 428 + 4 437 697 = 4 787 125, qs_net first, then po_net as efe_dec_grad lays it
 * out: the order torch.optim.Adam(model_down.parameters()) sees.  efe_adam_step and efe_get_weights refuse both names: the optimiser
 * step of "down" has functions of its own (efe_train_down, efe_down_adam_step, efe_down_get_weights below).
 *   efe_enc_grad  : the vector-Jacobian product of the encoder for the upstream pair g_mean, g_logvar [M,10]:
 *                   grad [349 428] = sum_r g_mean_r . d mean_r / d parameters + g_logvar_r . d logvar_r / d parameters.
 *                   o [M,1,64,64], g_mean, g_logvar, nz and grad are required.  nz keys the three dropout masks: the FORWARD encoder's,
 *                   draw for draw (tag TAG_ENC + layer, global row row_offset + r, stream_id(pass, sample), stage), so efe_encoder with the
 *                   same efe_noise encodes the same network: mean / logvar [M,10] agree with it to rounding, not bit for bit.  Optional
 *                   outputs (NULL = not wanted): mean, logvar, the stored activations y1 [M,32,31,31], y2 [M,32,15,15], y3 [M,64,7,7],
 *                   y4 [M,64,3,3] (NCHW, after the ReLU) and h1, h2, h3 [M,256] (after the mask), whose sign is the backward gate.
 *   efe_down_grad : F_down and grad [4 787 125] = d mean(F_down) / d every parameter of ModelDown.  Per 64-row group: the encoder's
 *                   training forward (o1 -> qs1_mean, qs1_logvar), qs1 = eps exp(qs1_logvar / 2) + qs1_mean (eps [M,10] injected, or
 *                   NULL: efe_loss_down's draw under TAG_EPS), efe_dec_grad's group at scale beta_o / M, the gradient of the loss at the
 *                   latent (g_mean, g_logvar [M,10], optional outputs; ps1_mean, ps1_logvar and omega are constants, as the reference
 *                   detaches them), and the encoder's backward.  params: gamma, beta_s, beta_o and omega_mode EFE_OMEGA_ARRAY or
 *                   EFE_OMEGA_SCALAR (EFE_OMEGA_DERIVED is refused).  out: F_down is required; nlogpo1, kl_s, kl_naive, po1, qs1,
 *                   qs1_mean, qs1_logvar are optional, the other fields are not read.  F_down and its terms are efe_loss_down's
 *                   expressions evaluated on the training forward, so they agree with efe_loss_down to rounding.  The po_net gradient,
 *                   po1 and nlogpo1 are bit-identical to efe_dec_grad(qs1, o1, scale < 0), the qs_net gradient to efe_enc_grad on the
 *                   returned upstream pair.
 * Both are fixed-order sums that depend on M alone: twice the same bits; the per-row outputs depend on that row and
 * its global row id only.  Scratch comes from the context's arena (on top of efe_dec_grad's: at most 21 MB of encoder activations and
 * gradients per group, 32 partial gradients of 260 KB and four of 1.1 MB).  Both return 1 with a message that names the function for
 * M <= 0, a NULL required pointer, a context of another geometry, or a split-operand option (mfma_bf16x3 / mfma_f16x2) being on. */
int efe_enc_grad(efe_ctx*, const float* o, const float* g_mean, const float* g_logvar, int M, const efe_noise* nz, float* mean, float* logvar,
                 float* grad, float* y1, float* y2, float* y3, float* y4, float* h1, float* h2, float* h3, void* stream);
int efe_down_grad(efe_ctx*, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                  const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, void* stream);

/* ---- the same gradient of F_down at every admitted geometry (csrc/train_enc_g.hip with the two run-time decoder files; additive to ABI 6) ----
 * efe_enc_grad's and efe_down_grad's arguments and meaning with the sizes taken from the context: C = 1..3 channels, resolution R,
 * conv extents H_l = (H_{l-1} - 3) / 2 + 1 from H_0 = R (84 -> 41, 20, 9, 4), K = 64 H4^2 inputs of qs_net.9 (64 .. 3 136):
 *   o, o1, po1 [M,C,R,R] (the caller's NCHW image, read directly)   y1 [M,32,H1,H1]  y2 [M,32,H2,H2]  y3 [M,64,H3,H3]  y4 [M,64,H4,H4]
 *   efe_param_count("qs_net_g") = 201 684 + 288 C + 256 K (9.weight is [256][K]); efe_param_count("down_g") = that + efe_param_count("po_net"),
 *   qs_net first.  ("qs_net" and "down" keep counting the 1 x 64 x 64 geometry only.)  efe_adam_step and efe_get_weights refuse both names.
 * They run kernels whose sizes are run-time values at EVERY geometry, 1 x 64 x 64 included (there efe_enc_grad / efe_down_grad are a
 * cross-check: both hold the fp64 rule; their bits are not promised equal).  The masks are the forward encoder's and decoder's at that
 * geometry.  A layer whose input extent is even never reads the last row and column of its input: the gradient there is an exact zero.
 * efe_down_grad_g queues per row group the encoder's forward, the sample, efe_dec_grad_g's group at scale beta_o / M, F_down's terms, the
 * gradient at the latent and the encoder's backward: the po_net gradient, po1 and nlogpo1 are bit-identical to efe_dec_grad_g(qs1, o1,
 * scale < 0), the qs_net gradient to efe_enc_grad_g on the returned upstream pair.  Fixed-order sums that depend on the geometry and M
 * alone: twice the same bits; per-row outputs depend on that row and its global row id only.  Rows are processed
 * in groups of 64 (resolution <= 64) or 32; scratch comes from the context's arena.  Both return 1 with a message that names the function,
 * before the first launch, for M <= 0, a NULL required pointer, a split-operand option (mfma_bf16x3 / mfma_f16x2) being on, or
 * EFE_OMEGA_DERIVED.  The optimiser step at these geometries: efe_train_down_g / efe_down_adam_step_g below. */
int efe_enc_grad_g(efe_ctx*, const float* o, const float* g_mean, const float* g_logvar, int M, const efe_noise* nz, float* mean, float* logvar,
                   float* grad, float* y1, float* y2, float* y3, float* y4, float* h1, float* h2, float* h3, void* stream);
int efe_down_grad_g(efe_ctx*, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                    const efe_noise* nz, const float* eps, efe_fe_out* out, float* g_mean, float* g_logvar, float* grad, void* stream);

/* ---- the optimiser step of ModelDown: train_model_down (csrc/train_down.hip; additive to ABI 6) -------------------------------------------
 * torch.optim.Adam's default update over the flat [4 787 125] parameter vector of ModelDown (the order of efe_down_grad's gradient), at the
 * 1 x 64 x 64 geometry.  The engine owns a master copy of these parameters that survives efe_commit_weights; the step writes it and then
 * rebuilds, on the device, every packed form the forward paths read (fragment orders, tap tables, the Winograd and F(2, 2) matrices, padded
 * bias tables): each holds exactly what a fresh commit of the new weights would have packed.  A later efe_set_weight of a "down." tensor or
 * efe_commit_weights first brings the host tensors up to date (one synchronisation), so a trained part is never reverted.  The first decoder
 * pass behind a step fetches po_net.19.bias (4 bytes, handed to its kernel by value) on its own stream and synchronises that stream once; it
 * cannot be captured into a graph, and a graph captured BEFORE a step holds the old bias by value: re-capture graphs after a step of ModelDown.
 * A step also invalidates split-operand planes left from an earlier mfma_bf16x3 / mfma_f16x2: turning the option on after a step first brings
 * the host tensors up to date and packs the planes from the trained weights.  For a handle that is not live these three return 1 and
 * efe_last_error names the function ("<function>: stale or invalid context handle") until the thread's next call.
 * The string-part calls keep refusing these parts: efe_adam_step / efe_get_weights know nothing of a repack; these are separate functions.
 *   efe_train_down      : efe_down_grad's groups, the update and the repack queued on the stream, no host synchronisation; bit-identical to
 *                         efe_down_grad followed by efe_down_adam_step.  out (as efe_down_grad's) reports the weights BEFORE the step.
 *   efe_down_adam_step  : update and repack from the caller's gradient [4 787 125]; exp_avg / exp_avg_sq [4 787 125] are the caller's state.
 *   efe_down_get_weights: the master copy -> dst (device), n == efe_param_count("down"), ordered on the stream.
 * Each returns 1 with a message that names the function for a NULL required pointer, M <= 0, hp NULL or hp->step < 1 (or other bad
 * hyper-parameters), EFE_OMEGA_DERIVED, a context of another geometry, or a split-operand option (mfma_bf16x3 / mfma_f16x2) being on; a
 * refused call changes no weight and no optimiser state.  Scratch (the gradient, on top of efe_down_grad's) comes from the context's arena. */
int efe_train_down(efe_ctx*, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                   const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream);
int efe_down_adam_step(efe_ctx*, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream);
int efe_down_get_weights(efe_ctx*, float* dst, int64_t n, void* stream);

/* ---- the same step at EVERY admitted geometry: train_model_down_g (csrc/train_down_g.hip behind k_adam_down; additive to ABI 6) ---------------
 * The three functions above with the sizes taken from the context: the flat vector has efe_param_count("down_g") floats (efe_down_grad_g's
 * order).  A context of any other geometry than 1 x 64 x 64 owns a master copy of its own that survives efe_commit_weights; the step writes
 * it and rebuilds, on the device, every packed form the generic forward path reads (the 32x32x2 and 16x16x4 fragment orders of the dense
 * layers, po_net.9 with its rows and qs_net.9 with its columns in NHWC order, nine-tap forms of the four Conv2d and three ConvTranspose2d
 * layers, the two small forms of qs_net.0 and po_net.19, padded bias tables): each holds exactly what a fresh commit of the new weights would
 * have packed.  efe_set_weight of a "down." tensor and efe_commit_weights first bring the host tensors up to date, as above.  The first
 * decoder pass behind a step fetches po_net.19.bias (C floats, handed to its kernel by value) on its own stream and synchronises that stream
 * once; it cannot be captured into a graph, and a graph captured before a step holds the old bias.  At 1 x 64 x 64 these functions run
 * efe_down_grad_g's kernels for the gradient and then THE SAME update and repack as the functions above, on the same master copy: the two
 * families may be mixed freely there.
 *   efe_train_down_g      : efe_down_grad_g's groups, the update and the repack queued on the stream, no host synchronisation; bit-identical
 *                           to efe_down_grad_g followed by efe_down_adam_step_g.  out reports the weights BEFORE the step.
 *   efe_down_adam_step_g  : update and repack from the caller's gradient; exp_avg / exp_avg_sq are the caller's state, all of "down_g" floats.
 *   efe_down_get_weights_g: the master copy -> dst (device), n == efe_param_count("down_g"), ordered on the stream.
 * Each returns 1 with a message that names the function, before the first launch, for M <= 0, a NULL required pointer, hp NULL or bad
 * hyper-parameters, EFE_OMEGA_DERIVED, a split-operand option being on, weights that are not committed, or a handle that is not live; a
 * refused call changes no weight, no optimiser state and no packed form.  efe_down_adam_step, efe_train_down and efe_down_get_weights keep
 * refusing every geometry but 1 x 64 x 64. */
int efe_train_down_g(efe_ctx*, const float* o1, const float* ps1_mean, const float* ps1_logvar, int M, const efe_fe_params* params,
                     const efe_noise* nz, const float* eps, efe_fe_out* out, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream);
int efe_down_adam_step_g(efe_ctx*, const float* grad, float* exp_avg, float* exp_avg_sq, const efe_adam_params* hp, void* stream);
int efe_down_get_weights_g(efe_ctx*, float* dst, int64_t n, void* stream);

/* ---- one whole training step: the loop body of the reference's train.py:111-126 (additive to ABI 6) --------------------------------------
 * One call, one call scope, everything queued on `stream`, no host synchronisation.  At the 1 x 64 x 64 geometry, in this order:
 *   1. qs0 = encoder_with_sample(o0)                              pass PASS_FE_Q0 (9):  encoder masks + normals (eps plane 0)
 *   2. the habit net's step (efe_train_top)                       -> kl_pi [M] of the weights before the step
 *   3. omega [M]: params->omega_mode EFE_OMEGA_DERIVED = compute_omega(kl_pi, a, b, c, d) on the device (train.py:118), the expression
 *      efe_free_energy evaluates; EFE_OMEGA_ARRAY / EFE_OMEGA_SCALAR: the caller's omega, copied to out->omega
 *   4. qs1_mean, qs1_logvar = encoder(o1)                         pass PASS_FE_Q1 (10): encoder masks
 *   5. the transition net's step (efe_train_mid)                  pass PASS_FE_T (11):  -> ps1_mean, ps1_logvar, F_mid before the step
 *   6. ModelDown's step (efe_train_down)                          pass PASS_FE_DOWN (12), eps plane 2: -> F_down, nlogpo1, kl_s, kl_naive
 * One stage (nz->stage) per call; nz->pass / nz->sample are not read; rows are keyed by global row nz->row_offset + r.
 * in->eps: NULL, or injected normals [3][M][s_dim] laid out as efe_free_energy's: plane 0 is the FE_Q0 sample, plane 2 the FE_DOWN
 * sample, plane 1 is not read (the training call draws no transition normals).
 * Each part brings its optimiser state and hyper-parameters (efe_step_adam; hp.step = that part's step number, 1 for its first step).
 * CONTRACT: bit-identical to efe_encoder(PASS_FE_Q0), efe_train_top, efe_encoder(PASS_FE_Q1), efe_train_mid(omega), efe_train_down(omega)
 * issued one after another with the same seed, stage and row_offset and the per-row omega of step 3: every output, the three master
 * copies, every packed forward form and all six state vectors.  The call runs those entry points' own launch sequences and adds no
 * summation of its own, so a step with derived omega equals a step given its own out->omega as EFE_OMEGA_ARRAY.
 * out->means (optional, EFE_STEP_MEANS floats): the batch means of kl_pi, omega, F_mid, F_down, nlogpo1, kl_s, kl_naive, then the
 * unbiased standard deviation of omega (train.py:158-159; NaN at M = 1, as torch.std) -- a fixed-order reduction that depends on M alone
 * (csrc/loss.hip k_step_means), so a loop can log its losses without synchronising every step.
 * Required: in and its o0, o1, pi0, log_Ppi; params; nz; top, mid, down with both state vectors; out with kl_pi and F_down.  Every
 * refusal comes before the first launch -- M < 1, a NULL required pointer, an unknown omega_mode or EFE_OMEGA_ARRAY without
 * params->omega, a geometry other than 1 x 64 x 64, a split-operand option (mfma_bf16x3 / mfma_f16x2) being on, hyper-parameters
 * efe_adam_step would refuse for any part -- with a message that names efe_train_step; a refused step changes no weight and no state.
 * Scratch comes from the context's arena (the three parts reuse it one after another). */
enum { EFE_STEP_MEANS = 8 };
typedef struct efe_step_in { const float* o0; const float* o1 /*[M,1,64,64]*/; const float* pi0; const float* log_Ppi /*[M,A]*/; const float* eps; } efe_step_in;
typedef struct efe_step_adam { float* exp_avg; float* exp_avg_sq; efe_adam_params hp; } efe_step_adam;
/* [M] unless stated; NULL = not wanted, except kl_pi and F_down */
typedef struct efe_step_out {
    float* kl_pi; float* omega; float* qs0 /*[M,s]*/; float* F_mid; float* ps1_mean /*[M,s]*/; float* ps1_logvar /*[M,s]*/;
    float* F_down; float* nlogpo1; float* kl_s; float* kl_naive; float* means /*[EFE_STEP_MEANS]*/;
} efe_step_out;
int efe_train_step(efe_ctx*, const efe_step_in* in, int M, const efe_fe_params* params, const efe_noise* nz, const efe_step_adam* top,
                   const efe_step_adam* mid, const efe_step_adam* down, const efe_step_out* out, void* stream);

/* ---- the epoch report: batch statistics of an evaluation batch (csrc/eval.hip; additive to ABI 6) -----------------------------------------
 * What the reference's train.py:136-187 appends to `stats` once an epoch, reduced on the device into ONE row of EFE_EVAL_STATS floats, in
 * one call scope with no host synchronisation and no scratch.  Row layout (s_dim 10, pi_dim 4, 6 true factors):
 *    0      F                  mean over rows of (F_down[r] + F_mid[r]) + F_top[r], the fp32 per-row sum in that order (train.py:149)
 *    1-6    F_top, F_mid, F_down, mse_o (= mean nlogpo1), kl_div_s, kl_div_s_naive                                batch means
 *    7-11   kl_div_pi mean, min, max, med, std: min / max / med return an input element, med is torch.median's lower median (the element
 *           of sorted rank (M - 1) / 2), std is unbiased, two passes as efe_train_step's omega_std, NaN at M = 1
 *    12     TC                 total correlation of a Gaussian fitted to qs1 (torchutils.py:40-42): (sum_k log cov_kk - log det cov) / 2, the
 *                              covariance with divisor M - 1, both terms from one Cholesky factor, all in fp64, rounded once to fp32.  A
 *                              non-positive pivot (a constant latent) or M <= 10 gives NaN, where numpy's slogdet route gives inf or a huge number
 *    13     mse_r              compare_reward (src/util.py:82-85): mean of (o1 - po1)^2 over image rows 0..2 of NCHW [Mr,1,64,64]
 *    14-23, 24-33, 34-37       kl_div_s_anal [10], kl_div_s_naive_anal [10], kl_div_pi_anal [4]                       column means
 *    38-97  spearman [10][6]   signed Spearman rho of s0[:, i] against S_real[:, j] (columns: shape, scale, orientation, posX, posY, reward),
 *                              ties at their average rank, from doubled integer ranks summed in int64 and ONE fp64 quotient: exactly what
 *                              the rank formula gives.  A constant column gives 0 / 0 = NaN, as scipy does
 * Inputs come in four groups, each all-or-nothing; an absent group leaves its fields NaN:
 *    FE  : F_top, F_mid, F_down, nlogpo1, kl_s, kl_naive, kl_pi [M]; kl_s_anal, kl_naive_anal [M,10]; kl_pi_anal [M,4]   -> 0-11, 14-37
 *    TC  : qs1 [M,10]                                                                                                    -> 12
 *    RHO : s0 [M,10], S_real [M,6]                                                                                       -> 38-97
 *    R   : o1_r, po1_r [Mr,1,64,64], Mr >= 1                                                                             -> 13
 * Every mean, the std and mse_r follow k_step_means' order contract (a function of the element count alone): thread t of a 256-thread
 * workgroup adds elements t, t + 256, ... in ascending order, xor butterfly over the wave (offsets 32 ... 1), ((w0 + w1) + w2) + w3, one
 * correctly rounded division.  Non-finite values: every field is NaN exactly where numpy / torch on the same arrays give NaN (min, max
 * and med propagate a NaN explicitly, a NaN in either column makes that rho NaN); a field that does not read a poisoned array keeps its bits.
 * Returns 1 with a message that names efe_eval_stats, before the first launch and writing nothing, for: in or out NULL, no group at all, a
 * partial group, M < 1, M > EFE_EVAL_MAX_ROWS, Mr > EFE_EVAL_MAX_ROWS (the cap: one column of M floats in LDS, 4 M^4 < 2^63). */
enum { EFE_EVAL_STATS = 98, EFE_EVAL_MAX_ROWS = 8192 };
typedef struct efe_eval_in {
    const float* F_top; const float* F_mid; const float* F_down; const float* nlogpo1; const float* kl_s; const float* kl_naive; const float* kl_pi;
    const float* kl_s_anal; const float* kl_naive_anal; const float* kl_pi_anal;      /* FE */
    const float* qs1;                                                                 /* TC */
    const float* s0; const float* S_real;                                             /* RHO */
    const float* o1_r; const float* po1_r; int Mr;                                    /* R */
} efe_eval_in;
int efe_eval_stats(efe_ctx*, const efe_eval_in* in, int M, float* out /*[EFE_EVAL_STATS]*/, void* stream);

/* ---- the epoch report: mutual information of latents and true factors (csrc/eval_mi.hip; additive to ABI 6) -------------------------------
 * The second curve of the reference's traversal figure (graphs/generate_traversals.py:36-46): out[l * 6 + f] = the mutual information of
 * latent column l of s0 [M][10] and factor column f of S_real [M][6], by the Kraskov-Stoegbauer-Grassberger k-nearest-neighbour estimator
 * as scikit-learn's mutual_info_regression defines it for float64 columns, in one call scope with no host
 * synchronisation.  Per pair, in fp64 with contraction off: each column is divided by its standard deviation (divisor M; 1 where it is
 * below 10 * 2^-52) and gets the jitter (1e-10 * max(1, mean|v|)) * noise; r_i is the n_neighbors-th smallest Chebyshev distance of point i
 * to another point, moved one fp64 step toward zero; nx_i, ny_i count the other points within r_i on each axis;
 * MI = max(0, psi(M) + psi(n_neighbors) - mean psi(nx + 1) - mean psi(ny + 1)), rounded once to fp32.
 *   noise  : [EFE_EVAL_MI][2][M] fp64, pair-major, the latent's vector first; or NULL: element 0 of the normal vector of counter
 *            (TAG_MI = 0x80, row i, stream_id(pair, which), stage) under the key of `seed`, widened to double (which: 0 latent, 1 factor).
 *            With device noise the result is a function of (s0, S_real, n_neighbors, seed, stage) alone.
 *   counts : NULL, or int32 [EFE_EVAL_MI][2][M]: nx then ny of every pair.
 * The sums behind the standard deviations and mean|v| follow efe_eval_stats' order contract with an fp64 accumulator; the last step has a
 * fixed order too, with psi from a table of harmonic numbers (csrc/eval_mi.hip), so the result is the same bits on every run.  A pair whose latent
 * column, factor column or noise holds a NaN or an infinity is NaN; the other pairs keep their bits.
 * Returns 1 with a message that names efe_eval_mi, before the first launch and writing nothing, for: in, out, in->s0 or in->S_real NULL,
 * n_neighbors outside 1 .. EFE_EVAL_MI_MAX_NEIGHBORS, M < n_neighbors + 1, M > EFE_EVAL_MAX_ROWS. */
enum { EFE_EVAL_MI = 60, EFE_EVAL_MI_MAX_NEIGHBORS = 4 };
typedef struct efe_eval_mi_in {
    const float* s0; const float* S_real; const double* noise;
    int n_neighbors; uint64_t seed; uint32_t stage;
} efe_eval_mi_in;
int efe_eval_mi(efe_ctx*, const efe_eval_mi_in* in, int M, float* out /*[EFE_EVAL_MI]*/, int32_t* counts, void* stream);

/* introspection for benches: algorithmic MACs of the last EFE-level call (0 for a handle that is not live). */
int64_t efe_last_call_macs(efe_ctx*);

/* per-kernel-class timing with HIP events recorded on the launch stream (bench.py roofline leg).
 * classes: 0 transition MLP, 1 decoder dense 10-256-256-256, 2 decoder dense 256->16384, 3 unused,
 * 4 k_dec_a (ConvT 64->64 s1 + ConvT 64->64 s2), 5 k_dec_b (ConvT 64->32 s2 + final conv + sigmoid + reductions),
 * 6 unused, 7 encoder, 8 other.
 * efe_prof_read synchronises the device, returns summed milliseconds and launch counts per class, and clears. */
int efe_prof_enable(efe_ctx*, int on);   /* 0 = off, < 0 = every class, otherwise a bitmask (bit c = class c) */
int efe_prof_classes(void);
int efe_prof_read(efe_ctx*, double* ms /*[classes]*/, int64_t* launches /*[classes]*/);

#ifdef __cplusplus
}
#endif
#endif
