/*
 * osdiff.h -- C ABI of libosdiff.so, the MI355X (gfx950) implementation of the
 * diffusion hot path of rare-resilience-ai/Osteosarcoma_DiffusionModel.
 *
 * The reference has no FFI boundary of its own: its hot path is the Python object
 * API of models/diffusion.py, utils/train.py and utils/generate.py.  Each entry
 * point below names the reference function (file:line, relative to the reference
 * tree) whose arithmetic it replaces; the Python shim in
 * osteosarcoma_diffusionmodel_amd/ keeps the reference's class and method names
 * and calls these through ctypes.
 *
 * Conventions
 *   - every function returns 0 (OSD_OK) or a negative OSD_E* code; no exceptions,
 *     no aborts.  osd_last_error() returns the message of the last failure on the
 *     calling thread.
 *   - all tensors are row-major contiguous fp32 unless stated; "dev" pointers are
 *     device memory of the handle's device, "host" pointers are host memory.
 *   - the caller owns every tensor; the library borrows pointers for the duration
 *     of a call, except the parameter pointers given to osd_load_weights(), which
 *     are borrowed until the next osd_load_weights() / osd_destroy().
 *   - all work is enqueued on the handle's stream (osd_set_stream) and is
 *     asynchronous unless stated; calls on one handle are not re-entrant.
 *   - no CPU fallback exists: without a HIP device every compute call fails.
 *   - row_offset (global id of the call's first row) addresses the Philox stream with
 *     32-bit row counters: row_offset < 0 or row_offset + n > 2^32 is OSD_EINVAL.
 *   - t_index entries must lie in [0, T): the reference's buffer gather raises
 *     IndexError otherwise (models/diffusion.py:337) and so does the Python shim; the
 *     library itself cannot see device values without a sync, so it clamps a
 *     caller-supplied t_index into [0, T) (no out-of-bounds table read can occur).
 */
#ifndef OSDIFF_H
#define OSDIFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSD_VERSION 100 /* 0.1.0 */

#define OSD_OK            0
#define OSD_EINVAL       -1 /* bad argument / shape (Python: ValueError)        */
#define OSD_ENOMEM       -2 /* allocation failed                                 */
#define OSD_EHIP         -3 /* HIP runtime error (Python: RuntimeError)          */
#define OSD_ESTATE       -4 /* call order: schedule / weights not loaded         */
#define OSD_EUNSUPPORTED -5 /* architecture outside what the kernels cover       */

#define OSD_MAX_HIDDEN 8

/* flags */
#define OSD_F_GRAPH      1 /* replay the reverse step from a captured hipGraph   */
#define OSD_F_TRAIN_MODE 2 /* dropout active (model.train())                     */
#define OSD_F_SYNC       4 /* synchronise the handle's stream before returning   */

typedef struct osd_handle osd_handle;

/* Constructor arguments of BiologyAwareDiffusionModel (models/diffusion.py:264-301). */
typedef struct osd_config {
  int32_t mutation_dim;
  int32_t expression_dim;
  int32_t pathway_dim;
  int32_t condition_dim;
  int32_t time_dim;                    /* config.model.latent_dim; cond width is time_dim/2 and must be 64 */
  int32_t n_hidden;                    /* len(config.model.hidden_dims)                    */
  int32_t hidden_dims[OSD_MAX_HIDDEN]; /* each divisible by 8 (GroupNorm(8, C))            */
  int32_t num_steps;                   /* config.model.diffusion.num_steps (T)             */
  float   dropout_p;                   /* config.model.gnn.dropout (models/diffusion.py:294)*/
  int32_t device;                      /* HIP device ordinal                                */
} osd_config;

int         osd_version(void);
const char *osd_last_error(void);

/* Number of trainable parameter tensors for this architecture (52 at n_hidden == 3),
 * in the order of BiologyAwareDiffusionModel.named_parameters(); 0 on bad config. */
int osd_num_params(const osd_config *cfg);
/* Element count of parameter i (same order); -1 on bad index. */
int64_t osd_param_numel(const osd_config *cfg, int i);

/* models/diffusion.py:264-310 (construction).  Allocates schedule tables and streams. */
int osd_create(const osd_config *cfg, osd_handle **out);
int osd_destroy(osd_handle *h);

/* Bind the HIP stream (hipStream_t, e.g. torch.cuda.current_stream().cuda_stream). */
int osd_set_stream(osd_handle *h, void *hip_stream);

/* Options: name -- accepted values (default) -- meaning.  osd_get_option reads each of them back.
 *
 * "sampler"                -- 0 | 1 | 2 (0) -- engine of the reverse chain: 0 auto (the chain kernel when the batch has at least as
 *                             many 128-row tiles as the device holds resident workgroups -- 65 536 rows on an MI355X -- or falls
 *                             into the window of the LDS-resident or squad chain, see "chain_variant", and the model is in eval
 *                             mode; else the per-layer kernels), 1 the persistent chain kernel wherever the architecture allows
 *                             it, 2 the per-layer kernels.
 * "chunk_rows"             -- >= 1 (65 536) -- per-layer path: rows per sampling chunk.
 * "n_streams"              -- 1..8 (2) -- per-layer path: chunks in flight.
 * "chain_variant"          -- 0..3 (0) -- which chain kernel: 1 the workspace chain, 128-row tiles whose activations pass through a
 *                             private workspace (the faster one from 65 536 rows on); 2 the LDS-resident chain, 64 patients per
 *                             workgroup with every activation in LDS, bit-identical, for architectures whose panels fit
 *                             (hidden_dims[0] = 256 = the last block's width; others fall back to 1), at its full rate from 16 384
 *                             rows on; 3 the squad chain, the small-batch kernel: eight workgroups per 32 patients for the whole
 *                             chain, for models it decomposes ("squad_chain_supported") and batches whose squads are all resident
 *                             (3 072 rows on 256 CUs), others run what auto would; it agrees with the other engines to fp32
 *                             rounding, not bitwise; 0 auto: 1 from 65 536 rows on, 2 from 10 240 rows on, 3 for resident batches
 *                             when "input_splitk" != 0.
 * "squad_panel"            -- 0 | 16 | 32 (0) -- patients per panel of the squad chain: 0 auto (16 up to 1 024 rows, 32 above).
 * "chain_grid"             -- 0..65 536 (0) -- cap on the chain kernel's workgroups; 0 = min(row tiles, resident slots).
 * "chain_steps_per_launch" -- >= 0 (0) -- steps of the chain per launch; 0 = the whole chain in one launch.
 * "chain_stagger"          -- 0..1e8 (30 000) -- shader cycles between the starts of the two workgroups of a CU; 0 = off.
 * "chain_spin_budget"      -- >= 0 (500 000 000 = 5 s) -- ticks of the 100 MHz s_memrealtime counter a dependency wait inside the
 *                             chain kernel may take.
 * "chain_wall_budget_ms"   -- >= 0 (0) -- host-side budget of a synchronous chain; 0 = 10 x the estimated run time + 2 s.
 * "input_splitk"           -- -1..64 (0) -- the small-batch mode of sampling: 0 off (a row's result does not depend on the batch it
 *                             is in, bit for bit), -1 auto, n > 0 slices: small batches run input_proj and the deep layers split
 *                             over K, or, where chain_variant 3 applies, the squad chain; another fp32 summation order, chain
 *                             tolerance against the default.
 * "precision"              -- 0 | 1 (0) -- 0 fp32 MFMA (the reference's arithmetic); 1 bf16x3 split on the bf16 matrix pipe (fp32
 *                             accuracy) for eval-mode sampling / forward of 256 / 512 wide trunks, OSD_EUNSUPPORTED elsewhere.
 * "train_streams"          -- 1 | 2 (2) -- 2: the weight-gradient leaves of a backward pass on a side stream; 1: one stream.
 * "train_squad"            -- 0..2 (2) -- from 2 048 rows on: 2 runs the ten Linear+GroupNorm+SiLU layers of a training forward pass
 *                             as one launch of squads (csrc/train_squad.h) and the dgrad chain of the backward pass as another
 *                             (csrc/train_squad_bwd.h; single-process steps only: bucket events keep the per-layer dgrads);
 *                             1 the forward only; 0 per-layer launches.
 * "cond_bwd_fused"         -- 0 | 1 (1) -- 1: the conditioning branch's backward below h0 (time-table scatter, two 64-wide dgrads,
 *                             SiLU backward, the first embedding Linear's weight gradient) as one launch, k_cond_bwd in
 *                             csrc/k_train.hip, for hidden_dims[0] <= 256 and a multiple of 32; 0: five launches.
 * "bound_rows"             -- 1..2^30 (32 768) -- rows per launch group of osd_bound_sweep / osd_row_sq_error / osd_noise_map: caps their workspace.
 *
 * Any other name: OSD_EINVAL. */
int osd_set_option(osd_handle *h, const char *name, int64_t value);

/* Reads an option back (see osd_set_option), or one of the read-only counters: "chain_fallbacks" (chains that gave up -- see
 * osd_sample_chain -- and were re-run on the per-layer kernels), "last_engine" (0 per-layer kernels, 1 chain kernel),
 * "last_chain_variant" (1 | 2 | 3, the chain kernel that ran last), "last_squad_panel" (patients per panel of the squad chain
 * that ran last), "last_precision" (0 | 1, what the most recent forward / p_sample / sample computed in), "split_supported"
 * (1 when "precision" 1 applies to this model), "panel_chain_supported" / "squad_chain_supported" (1 when "chain_variant"
 * 2 / 3 applies to this model), "last_train_path" (what the most recent osd_train_loss_fwd_bwd or osd_denoiser_backward call on
 * the handle ran, an OR of the OSD_TP_* bits below; cleared at the start of either call), "prediction_type" (OSD_PRED_*, what
 * osd_set_prediction set last; 0 on a new handle), "loss_mask" (0 | 1, what osd_set_loss_mask set last), "output_link" (n_logistic, what
 * osd_set_output_link set last; 0 on a new handle).  Any other name: OSD_EINVAL. */
int osd_get_option(osd_handle *h, const char *name, int64_t *value);

/* "last_train_path" bits */
#define OSD_TP_SQUAD_FWD     (1 << 0)   /* the forward trunk ran as one launch of squads (csrc/train_squad.h) */
#define OSD_TP_SQUAD_BWD     (1 << 1)   /* the backward dgrad chain ran as one launch of squads (csrc/train_squad_bwd.h) */
#define OSD_TP_FUSED_GN_BWD  (1 << 2)   /* GroupNorm backward inside the dgrad epilogues (else the stand-alone GroupNorm backward) */
#define OSD_TP_DUAL_DGRAD    (1 << 3)   /* at least one dgrad carried a skip connection's share in the same launch */
#define OSD_TP_COND_BWD      (1 << 4)   /* the conditioning branch's backward as one launch (k_cond_bwd; else five launches) */
#define OSD_TP_COND_BWD_CE0  (1 << 5)   /* ... with the first embedding Linear's weight gradient inside it */
#define OSD_TP_X_PADDED      (1 << 6)   /* x_t rows padded to whole K steps; input_proj read input_proj.weight itself */
#define OSD_TP_INPUT_REPACK  (1 << 7)   /* ... which it refused (unaligned weight): the padded copy was packed after all */
#define OSD_TP_WGRAD_DIRECT  (1 << 8)   /* at least one weight gradient launched on its own, outside the grouped launch */
#define OSD_TP_WGRAD_GROUP   (1 << 9)   /* at least one grouped weight-gradient launch */
#define OSD_TP_MSE_BF16      (1 << 10)  /* output_proj + MSE on the bf16 matrix pipe ("precision" 1) */
#define OSD_TP_LOSS_EPI      (1 << 11)  /* output_proj ran the configurable loss epilogue (osd_set_loss); never set on the default path */
#define OSD_TP_TARGET        (1 << 12)  /* q_sample wrote a non-eps training target (osd_set_prediction); never set on the default path */
#define OSD_TP_DP_CLIP       (1 << 13)  /* per-row gradient clipping ran (osd_set_dp_clip); never set on the default path */
#define OSD_TP_MASKED        (1 << 14)  /* NaN-masked q_sample and loss epilogue ran (osd_set_loss_mask); never set on the default path */
#define OSD_TP_LINK          (1 << 15)  /* the loss epilogue with the logistic link ran (osd_set_output_link); never set on the default path */

/* Schedule + time-embedding tables, computed by the host with the reference's own
 * fp32 expressions so they are bit-identical (models/diffusion.py:299-326, 131-137,
 * 401-419).  All host pointers:
 *   sqrt_ac[T], sqrt_1m_ac[T]   buffers used by q_sample (:337-338)
 *   post_coef[T*6]              per-step scalars of p_sample (:401-419), layout of
 *                               oracle/diffusion_oracle.py:posterior_coefficients
 *   time_emb[T*time_dim]        TimeEmbedding(t/T) rows for t = 0..T-1 (:131-137) */
int osd_set_schedule(osd_handle *h, const float *sqrt_ac, const float *sqrt_1m_ac,
                     const float *post_coef, const float *time_emb);

/* nn.Module parameters (models/diffusion.py:283-295): n == osd_num_params() device
 * pointers in named_parameters() order.  Borrowed; derived tables (time_proj applied
 * to the time-embedding table, packed / plane copies of weights) are recomputed on the
 * handle's stream.  Call again after any in-place parameter update the library cannot
 * see (an update through osd_clip_adamw_step on this handle, or a training call that
 * skipped a repack, is seen: the next forward / sampling entry point refreshes the
 * derived copies itself). */
int osd_load_weights(osd_handle *h, const float *const *params, int n);

/* DiffusionUNet.forward in eval/train mode on n rows (models/diffusion.py:210-256)
 * including ConditionalEmbedding (:101-114):  eps[n][D].
 *   t_index  dev int32[n] per-row timestep index, or NULL -> every row uses t_all
 *   masks    train mode only: dev float 0/1 keep-masks, one [n][C] per block in
 *            execution order (n_blocks pointers, host array), or NULL -> Philox(seed) */
int osd_denoiser_forward(osd_handle *h, const float *x, const int32_t *t_index, int32_t t_all,
                         const float *cond, int64_t n, float *eps, int flags,
                         const float *const *masks, uint64_t seed);

/* q_sample (models/diffusion.py:328-342): x_t = sqrt_ac[t]*x0 + sqrt_1m_ac[t]*noise.
 * noise_in NULL -> Philox(seed, row_offset) normals, written to noise_out. */
int osd_q_sample(osd_handle *h, const float *x0, const int32_t *t_index, const float *noise_in,
                 int64_t n, uint64_t seed, int64_t row_offset, float *x_t, float *noise_out);

/* ---- what the network predicts ------------------------------------------------------------------------------------------
 * With a = sqrt_ac[t], b = sqrt_1m_ac[t] and `out` the network's raw output:
 *   OSD_PRED_EPSILON  target eps                 x0^ = (1/a) x_t - (b/a) out     (the reference's; the state of a new handle)
 *   OSD_PRED_V        target a*eps - b*x0        x0^ = a x_t - b out             (Salimans & Ho 2022)
 *   OSD_PRED_SAMPLE   target x0                  x0^ = out
 * x0^ = P x_t + Q out.  The training target is formed inside the q_sample kernels of osd_train_loss_fwd_bwd (fp32: two rounded
 * products and one subtraction for v) and the loss compares the output with it; such a call sets OSD_TP_TARGET.  The constraint
 * losses take x0^ from a device table [T][2] of (P, Q).  Every reverse step is x' = E x0^ + F x_t + C z with E, F, C independent of the
 * type, so the DDPM rows of osd_p_sample_step / osd_sample_chain* are refolded as A = E P + F, B = E Q (float64 from the schedule's
 * fp32 scalars, rounded once) together with the (P, Q, E, F) rows of the clipped chain: every engine follows the type through its
 * tables.  Strided plans (osd_sample_chain_steps and the options' steps arguments) carry the caller's rows: fold them for the same type
 * (ddim.py).  Guidance combines raw outputs, which is guidance in eps-space for every type (all three readings of eps are affine
 * in `out`, the x_t term cancels).
 * Persistent like osd_set_loss; synchronises the handle's stream.  OSD_PRED_EPSILON restores the tables osd_set_schedule folded, bit
 * for bit; a later osd_set_schedule folds for the current type.  OSD_ESTATE before osd_set_schedule, OSD_EINVAL for an unknown type. */
#define OSD_PRED_EPSILON 0
#define OSD_PRED_V       1
#define OSD_PRED_SAMPLE  2
int osd_set_prediction(osd_handle *h, int type);

/* osd_q_sample that writes the current type's training target where osd_q_sample writes the noise: target_out dev [n][D], required,
 * distinct from noise_in and x0.  For OSD_PRED_EPSILON it is osd_q_sample (target_out = the noise).  Under osd_set_loss_mask it returns
 * what the training call forms: x_t of the zero-filled x0 and the target with NaN at the unobserved elements, for every type; target_out
 * must then be a buffer of its own for OSD_PRED_EPSILON too. */
int osd_q_sample_target(osd_handle *h, const float *x0, const int32_t *t_index, const float *noise_in,
                        int64_t n, uint64_t seed, int64_t row_offset, float *x_t, float *target_out);

/* Row-affine conversion of a raw output of the current type: dst[r] = U[t_r] x_t[r] + V[t_r] out[r], as_kind OSD_PRED_* naming what
 * dst is (OSD_PRED_SAMPLE: x0^ = P x_t + Q out; OSD_PRED_EPSILON: (x_t - a x0^)/b; OSD_PRED_V: a eps^ - b x0^).  (U, V) are formed in
 * float64 from the schedule's fp32 buffers and rounded once.  t_index dev int32[n]; dst may alias out. */
int osd_convert_prediction(osd_handle *h, const float *x_t, const int32_t *t_index, const float *out, int64_t n, int as_kind,
                           float *dst);

/* p_sample (models/diffusion.py:382-425): one reverse step at python-int t.
 * z NULL -> Philox(seed,row_offset,t).  In-place (x_out == x_t) is allowed. */
int osd_p_sample_step(osd_handle *h, const float *x_t, int32_t t, const float *cond, const float *z,
                      int64_t n, uint64_t seed, int64_t row_offset, float *x_out, int flags);

/* sample (models/diffusion.py:427-449) + binarisation of utils/generate.py:135.
 *   x_T     dev [n][D] start noise or NULL -> Philox
 *   noises  dev [T-1][n][D] in draw order (t = T-1 .. 1) or NULL -> Philox
 *   x_out   dev [n][D]
 *   mut_mask_out  dev float [n][mutation_dim] = (x_out[:, :mutation_dim] > 0.5) or NULL
 * Rows are split into chunks that run the whole T-step chain independently on the
 * handle's internal streams; row_offset makes Philox draws independent of sharding. */
int osd_sample_chain(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                     const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                     float *mut_mask_out, int flags);
/* Two engines run osd_sample_chain with identical results: the per-layer kernels (12 launches per step, replayed from a
 * hipGraph under OSD_F_GRAPH) and, for >= ~50 000 rows of an architecture with 256/512-wide blocks in eval mode, ONE
 * persistent kernel that carries each 128-row tile through all layers and all T steps (csrc/chain.h).  Returns the
 * engine a call with these n / flags would use (0 per-layer, 1 chain kernel); n < 0: the engine of the last call.  The
 * chain kernel bounds every inter-workgroup wait ("chain_spin_budget"), and a synchronous call bounds the kernel itself
 * ("chain_wall_budget_ms": hipStreamQuery poll, then an abort flag the waits observe).  If the chain gives up its results are
 * invalid: under OSD_F_SYNC the SAME call re-runs the chain on the per-layer kernels from x_T / seed (bit-identical results;
 * returns OSD_OK, osd_last_error() holds a warning, "chain_fallbacks" counts, osd_sample_engine(h, -1, 0) then reports 0) --
 * models/diffusion.py:427-449 cannot fail; without OSD_F_SYNC the next osd_sample_chain on the handle returns OSD_EHIP.
 * OSD_EHIP from a synchronous call means the kernel did not even react to the abort flag (device hung). */
int osd_sample_engine(osd_handle *h, int64_t n, int flags);

/* osd_sample_chain over a caller-supplied step plan of n_steps <= T steps (strided DDIM sampling, Song et al. 2021).  Both
 * arrays are on the host:
 *   timesteps  [n_steps]     tau_s, the schedule timestep step s evaluates the denoiser at (its time-embedding row)
 *   step_coef  [n_steps][4]  (A_s, B_s, C_s, 0): step s computes x' = A_s*x + B_s*eps + C_s*z with eps = denoiser(x, tau_s)
 * The chain runs s = n_steps-1 first, down to s = 0.  x_T comes from the same Philox stream as osd_sample_chain's (step counter
 * T), so the same seed / row_offset starts both from the same x_T; z of step s uses step counter s (so does train-mode dropout),
 * and step 0 draws no z.  noises: dev [n_steps-1][n][D] in draw order s = n_steps-1 .. 1, or NULL -> Philox.  mut_mask_out is
 * written by step 0.  Rows, chunks, engines and the OSD_F_SYNC re-run of a chain that gave up are those of osd_sample_chain;
 * the identity plan (tau_s = s, the schedule's own A_t, B_t, C_t) computes its bits.  The library folds nothing: for DDIM from
 * tau = tau_s to tau' = tau_{s-1} (abar' = 1 at s = 0) with abar = alphas_cumprod,
 *   x0^ = (x - sqrt(1-abar)*eps) / sqrt(abar),  x' = sqrt(abar')*x0^ + sqrt(1 - abar' - sigma^2)*eps + sigma*z
 *   sigma = eta * sqrt((1-abar') / (1-abar)) * sqrt(1 - abar/abar')
 *   =>  A = sqrt(abar'/abar),  B = sqrt(1 - abar' - sigma^2) - sqrt(abar')*sqrt(1-abar)/sqrt(abar),  C = sigma
 * (osteosarcoma_diffusionmodel_amd/ddim.py builds this plan).  OSD_EINVAL: n_steps outside [1, T], a tau outside [0, T), a
 * non-finite coefficient, or C_0 != 0. */
int osd_sample_chain_steps(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                           const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                           float *mut_mask_out, int flags, const int32_t *timesteps,
                           const float *step_coef, int32_t n_steps);

/* Classifier-free guidance (Ho & Salimans 2022) -- the guidance_scale of SyntheticPatientGenerator.generate (utils/generate.py:97-110:
 * "Guidance strength for conditional generation"; config/config.yaml:120 ships 7.5), which the reference accepts and never uses.
 * With the null condition c0 = null_cond_host (host, [condition_dim]; it goes through the unchanged ConditionalEmbedding and cond_proj,
 * models/diffusion.py:101-114, 226, like any other condition) and w = guidance_scale, every step of the chain steps on
 *   eps_g(x, t, c) = eps(x, t, c0) + w * (eps(x, t, c) - eps(x, t, c0))
 * in place of eps(x, t, c): w = 1 is osd_sample_chain / osd_sample_chain_steps, w = 0 the unconditional sampler.  timesteps == NULL:
 * the DDPM chain (step_coef / n_steps ignored); otherwise the arguments and checks of osd_sample_chain_steps.  x_T and every z come
 * from the Philox addresses of the unguided chain.  Per chunk of m rows a step is one input_proj product with two outputs (it does
 * not depend on the condition), the Linear+GroupNorm+SiLU layers on 2 m rows, the combination h_u + w * (h_c - h_u) on the last
 * hidden activation (output_proj is linear) and ONE output_proj + posterior launch over m rows.  Per-layer kernels only, whatever
 * "sampler" says (osd_sample_engine(h, -1, 0) then reports 0; no warning, "chain_fallbacks" untouched); a row's result does not
 * depend on the chunk or shard it is in ("input_splitk" = 0).  guidance_scale == 1.0f exactly takes the unguided entry point's
 * path: any engine, its bits.  OSD_EINVAL: non-finite guidance_scale or null_cond, OSD_F_TRAIN_MODE (no dropout inside a guided
 * chain); OSD_EUNSUPPORTED: "precision" = 1. */
int osd_sample_chain_guided(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                            const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                            float *mut_mask_out, int flags, const int32_t *timesteps,
                            const float *step_coef, int32_t n_steps, const float *null_cond_host,
                            float guidance_scale);

/* Known-feature conditioning: the chain samples around observed values (the replacement method of Song et al. 2021; RePaint without
 * its resampling loops).  known: dev [n][ld_known], a finite value is an observation of that element, NaN leaves it to the chain.
 * Step s of the plan goes from tau_s to tau' = tau_{s-1} (abar' = 1 at s = 0); with La_s = sqrt(abar'), Ls_s = sqrt(1 - abar'):
 *   free  element:  x' = A_s*x + B_s*eps + C_s*z          the unconstrained step, operation for operation
 *   known element:  x' = fmaf(La_s, known, Ls_s*z)        s > 0;   s == 0:  x' = known, bit for bit
 * z is the step's posterior draw at the element's own address: Philox (seed, row_offset + row, f/4, step counter s), or the caller's
 * noises[n_steps-1-s] -- a replaced element has no other use for it.  Every step with s > 0 draws z, also where C_s == 0 (eta = 0: the
 * free elements add exactly zero there), so noises is read at eta = 0 too and an all-NaN known gives the unconstrained per-layer
 * chain's bits.  Step 0 draws nothing; x_T is the unconstrained chain's and is not replaced (abar_{T-1} ~ 0).  mut_mask_out is
 * (x_out > 0.5) as ever: for an observed mutation of 0 or 1, the observation.
 *   timesteps == NULL   the DDPM chain (step_coef / known_level / n_steps ignored); the levels are the schedule's own buffers,
 *                       (sqrt_ac[s-1], sqrt_1m_ac[s-1]) as osd_set_schedule received them
 *   otherwise           osd_sample_chain_steps' plan and, host, known_level [n_steps][2] = (La_s, Ls_s), row 0 = (1, 0).  The library
 *                       folds nothing (ddim.py: known_level_table gathers the rows from the fp32 schedule buffers)
 *   null_cond_host == NULL  unguided (guidance_scale ignored); otherwise osd_sample_chain_guided's guided step, same output launch
 * One fused output_proj + posterior launch per step (EpiPosterior<POST_PLAIN, true>); per-layer kernels only, whatever "sampler" says
 * (osd_sample_engine(h, -1, 0) then reports 0; no warning, "chain_fallbacks" untouched); a row's result does not depend on the chunk
 * or shard it is in ("input_splitk" = 0).  OSD_F_TRAIN_MODE is allowed for unguided chains (the trunk is the unconstrained chain's).
 * OSD_EINVAL: known == NULL, ld_known < D, known_level[0] != (1, 0), a non-finite level, and everything osd_sample_chain_steps /
 * osd_sample_chain_guided reject; OSD_EUNSUPPORTED: "precision" = 1. */
int osd_sample_chain_known(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                           const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                           float *mut_mask_out, int flags, const int32_t *timesteps,
                           const float *step_coef, const float *known_level, int32_t n_steps,
                           const float *null_cond_host, float guidance_scale, const float *known,
                           int64_t ld_known);

/* The same chains with the predicted clean sample clipped to per-feature bounds inside the posterior launch (clip_denoised of
 * improved-diffusion / guided-diffusion, clip_sample of diffusers; static thresholding).  lo_host / hi_host: host [D], -inf / +inf
 * leave a side free.  Step s of the plan goes from tau_s to tau' = tau_{s-1} (abar' = 1 at s = 0); with abar = alphas_cumprod[tau_s],
 * sigma as in osd_sample_chain_steps and dir = sqrt(max(1 - abar' - sigma^2, 0)):
 *   P = 1/sqrt(abar)                               Q = -sqrt(1-abar)/sqrt(abar)
 *   E = sqrt(abar') - dir*sqrt(abar)/sqrt(1-abar)   F = dir/sqrt(1-abar)          C = sigma
 *   eps = denoiser(x, tau_s)                       (guided: osd_sample_chain_guided's eps_g)
 *   x0  = fmaf(P, x, Q*eps)
 *   x0c = fminf(fmaxf(x0, lo[f]), hi[f])
 *   x'  = fmaf(E, x0c, fmaf(F, x, C*z))            = sqrt(abar')*x0c + dir*(x - sqrt(abar)*x0c)/sqrt(1-abar) + sigma*z
 * The direction term uses the eps the CLIPPED x0 implies, not the network's.  Row 0 is (P, Q, 1, 0) with C_0 = 0, so x' = x0c bit for
 * bit: every returned element lies inside [lo, hi] exactly; mut_mask_out stays (x_out > 0.5).  Clamping the state x' instead is another
 * (wrong) algorithm, which is why this is an epilogue of the output_proj launch (EpiPosterior<POST_CLIP>, csrc/epilogues.h) and no pass of
 * its own.  Arguments and checks of osd_sample_chain_known, except:
 *   known == NULL       nothing is observed (known_level / ld_known ignored); otherwise observed elements are overwritten after the
 *                       clipped update with osd_sample_chain_known's expressions and draw rule (an observation outside the bounds
 *                       comes back as observed)
 *   x0_coef             host [n_steps][4] = (P_s, Q_s, E_s, F_s), row 0 = (., ., 1, 0) (ddim.py: ddim_x0_table).  step_coef supplies C_s
 *                       in slot 2; its A_s, B_s are validated as ever and not used
 *   timesteps == NULL   the DDPM chain (step_coef / x0_coef / known_level / n_steps ignored): p_sample (models/diffusion.py:398-425)
 *                       with x_0_pred clamped.  From osd_set_schedule's post_coef (c0 .. c5), folded in double and rounded once:
 *                       (P, Q, E, F, C) = (1/c1, -c0/c1, c2/c3, c4/c3, c5), and (1/c1, -c0/c1, 1, 0, 0) at t = 0
 * One fused output_proj + posterior launch per step; per-layer kernels only, whatever "sampler" says (osd_sample_engine(h, -1, 0) then
 * reports 0; no warning, "chain_fallbacks" untouched); a row's result does not depend on the chunk or shard it is in ("input_splitk"
 * = 0).  OSD_F_TRAIN_MODE is allowed for unguided chains.  All-infinite bounds agree with the unclipped chain to fp32 rounding, not
 * bitwise (another operation order).  OSD_EINVAL, checked on the host before any device call: a NULL bound, a NaN bound, lo[f] > hi[f],
 * a NULL or non-finite x0_coef, x0_coef[0] != (., ., 1, 0), and everything osd_sample_chain_known (with known != NULL),
 * osd_sample_chain_guided and osd_sample_chain_steps reject; OSD_EUNSUPPORTED: "precision" = 1. */
int osd_sample_chain_clipped(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                             const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                             float *mut_mask_out, int flags, const int32_t *timesteps,
                             const float *step_coef, const float *x0_coef, const float *known_level,
                             int32_t n_steps, const float *null_cond_host, float guidance_scale,
                             const float *known, int64_t ld_known, const float *lo_host,
                             const float *hi_host);

/* The DDIM chains at eta = 0 with the DPM-Solver++(2M) multistep update (Lu et al. 2022, the data-prediction form): every step also
 * uses the previous step's clipped x0, which the chain keeps in a buffer of its own beside the state.  Step s of the plan goes from
 * tau_s to tau' = tau_{s-1}, s = n_steps - 1 first; with alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = ln(alpha / sigma),
 * h_s = lambda' - lambda and phi = -alpha' * expm1(-h_s):
 *   row n_steps-1 (first run), every row when n_steps <= 2:   F = sigma'/sigma,  G = phi,               H = 0
 *   rows 0 < s < n_steps-1:  r = (lambda_s - lambda_{s+1}) / h_s,  F = sigma'/sigma,  G = phi*(1 + 1/(2r)),  H = -phi/(2r)
 *   row 0 (lower-order final; h = inf):                       F = 0,             G = 1,                 H = 0
 *   eps = denoiser(x, tau_s)                       (guided: osd_sample_chain_guided's eps_g)
 *   x0  = fmaf(P, x, Q*eps)                        (P, Q) as in osd_sample_chain_clipped
 *   x0c = fminf(fmaxf(x0, lo[f]), hi[f])
 *   x'  = fmaf(G, x0c, fmaf(F, x, H*x0c_prev))     x0c_prev: the x0c of the step run before this one (never read where H = 0)
 * G + H and F are the E and F of osd_sample_chain_clipped at eta = 0, so n_steps <= 2 is that chain.  Row 0 returns x0c bit for bit:
 * every returned element lies inside [lo, hi] exactly; mut_mask_out stays (x_out > 0.5).  Deterministic after x_T: there is no z, and
 * no step_coef.  The history is an epilogue stream of the output_proj launch (EpiPosterior<POST_HIST>, csrc/epilogues.h) because neither
 * x0c nor eps is ever written by it.  Arguments and checks of osd_sample_chain_clipped, except:
 *   timesteps           required: a solver needs a plan (NULL is OSD_EINVAL)
 *   x0_coef             host [n_steps][4] = (P_s, Q_s, G_s, F_s), row 0 = (., ., 1, 0);  hist_coef: host [n_steps] = H_s,
 *                       hist_coef[0] = hist_coef[n_steps-1] = 0 (ddim.py: dpmpp_2m_table)
 *   lo_host == hi_host == NULL   unbounded: the library fills (-inf, +inf) rows; one of the two NULL is OSD_EINVAL
 *   known != NULL       observed elements are overwritten after the update with osd_sample_chain_known's expressions and draw rule;
 *                       the history keeps the clipped network prediction, not the overwritten value.  noises [n_steps-1][n][D] (or
 *                       Philox) feeds only the observed elements, as in the eta = 0 known chain
 * One fused output_proj + update launch per step; per-layer kernels only, whatever "sampler" says (osd_sample_engine(h, -1, 0) then
 * reports 0; no warning, "chain_fallbacks" untouched); a row's result does not depend on the chunk or shard it is in ("input_splitk"
 * = 0).  OSD_F_TRAIN_MODE is allowed for unguided chains.  OSD_EINVAL, checked on the host before any device call: timesteps == NULL,
 * a NULL or non-finite x0_coef or hist_coef, x0_coef[0] != (., ., 1, 0), hist_coef[0] != 0, hist_coef[n_steps-1] != 0, exactly one
 * NULL bound, and everything osd_sample_chain_clipped, osd_sample_chain_known (with known != NULL), osd_sample_chain_guided and
 * osd_sample_chain_steps reject; OSD_EUNSUPPORTED: "precision" = 1. */
int osd_sample_chain_multistep(osd_handle *h, const float *cond, int64_t n, const float *x_T,
                               const float *noises, uint64_t seed, int64_t row_offset, float *x_out,
                               float *mut_mask_out, int flags, const int32_t *timesteps,
                               const float *x0_coef, const float *hist_coef, const float *known_level,
                               int32_t n_steps, const float *null_cond_host, float guidance_scale,
                               const float *known, int64_t ld_known, const float *lo_host,
                               const float *hi_host);

/* eps_g of ONE guided evaluation (DiffusionUNet.forward twice, models/diffusion.py:210-256, combined as above), eval mode only:
 * osd_denoiser_forward's x / t_index / t_all / cond / eps, osd_sample_chain_guided's null_cond_host / guidance_scale and errors. */
int osd_denoiser_forward_guided(osd_handle *h, const float *x, const int32_t *t_index, int32_t t_all,
                                const float *cond, int64_t n, float *eps, int flags,
                                const float *null_cond_host, float guidance_scale);

/* Condition dropout, the training side of classifier-free guidance (utils/train.py:230-236 hands the batch's conditions to the model
 * as they are; the unconditional branch of a guided sampler needs a model that has seen the null condition).  One-shot like
 * osd_train_batch_source: in the NEXT osd_train_loss_fwd_bwd on this handle, row i's condition is replaced by null_cond_host
 * (host, [condition_dim]) unless the row keeps it -- after the mixup of a resident batch source, before anything else reads it:
 *   keep_dev != NULL  dev float[n]: row i keeps its condition iff keep_dev[i] != 0
 *   keep_dev == NULL  row i keeps it iff u >= p, u = (w >> 8) * 2^-24 of word 0 of the Philox block at counter
 *                     (row_offset + i, 0, 0, tag 0x44524f80), key = that call's seed: the dropout keep-mask's construction with
 *                     one column per row, independent of sharding and predictable from the host
 * p == 0 with keep_dev == NULL clears the option: the next call draws nothing and launches nothing new.  Pure data movement: forward,
 * backward and the constraint losses see the replaced conditions and are otherwise unchanged. */
int osd_train_condition_dropout(osd_handle *h, const float *null_cond_host, double p, const float *keep_dev);

/* Device-resident epoch path (utils/train.py:204-250 hands every batch over from host memory; here the dataset of
 * OsteosarcomaDataset (utils/train.py:22-82) stays in HBM).  The NEXT osd_train_loss_fwd_bwd on this handle takes its n rows
 * from the dataset instead of its x0 / cond arguments (pass NULL there):
 *   row i  = lam * data[idx_a[i]] + (1 - lam) * data[idx_b[i]]      MixupAugmentation, utils/train.py:117-119, the two
 *            products rounded separately as torch evaluates them; conditions likewise
 *   idx_b NULL: no mixup;  idx_a NULL: rows 0 .. n-1.  idx_a / idx_b: dev int64[n].  One-shot: consumed by that call.
 * Gather, mixup, the draw of t and q_sample run as ONE pass over the batch (SURVEY a5 + a11). */
int osd_train_batch_source(osd_handle *h, const float *data, int64_t ld_data, const float *cond, int64_t ld_cond,
                           const int64_t *idx_a, const int64_t *idx_b, double lam);

/* Training forward+backward (models/diffusion.py:344-380 + loss.backward(),
 * utils/train.py:236-239): loss (dev float[1]) and gradients of all parameters.
 *   t_index   dev int32[n] or NULL -> Philox randint
 *   noise     dev [n][D] or NULL -> Philox
 *   masks     keep-masks as in osd_denoiser_forward, or NULL -> Philox / none in eval
 *   grads     n_params device pointers (host array); overwritten (not accumulated)
 *   loss_scale  multiplies the gradients (1.0 for plain backward)
 *   events/n_events  optional hipEvent_t array recorded on the handle's stream as
 *             each gradient bucket (see osd_grad_bucket) becomes final, for
 *             overlapping the RCCL all-reduce with the rest of backward
 * The loss is the MSE of the predicted noise unless osd_set_loss chose another one (L1, Huber, per-timestep weights). */
int osd_train_loss_fwd_bwd(osd_handle *h, const float *x0, const float *cond, int64_t n,
                           const int32_t *t_index, const float *noise, const float *const *masks,
                           uint64_t seed, int64_t row_offset, int flags, float *loss_out,
                           float *const *grads, double loss_scale, void *const *events, int n_events);

/* The same network split at the loss, for losses other than the eps-MSE (config.yaml:47 names l1 / huber):
 * osd_denoiser_forward_train is osd_denoiser_forward with per-row t_index that keeps the activations in the
 * handle's training workspace (valid until the next training call on the handle); osd_denoiser_backward takes an
 * arbitrary upstream gradient dout[n][D] = dL/d eps and writes every parameter gradient (overwritten) and, when
 * dx_t != NULL, dL/dx_t [n][D].  x_t, t_index, cond, masks / seed / row_offset and flags must be the forward call's. */
int osd_denoiser_forward_train(osd_handle *h, const float *x_t, const int32_t *t_index, const float *cond,
                               int64_t n, const float *const *masks, uint64_t seed, int64_t row_offset,
                               int flags, float *eps_out);
int osd_denoiser_backward(osd_handle *h, const float *x_t, const int32_t *t_index, const float *cond, int64_t n,
                          const float *dout, const float *const *masks, uint64_t seed, int64_t row_offset,
                          int flags, float *const *grads, float *dx_t, void *const *events, int n_events);

/* Gradient buckets in the order backward finalises them: bucket b covers parameters
 * [first, last] (indices in named_parameters() order).  Returns the bucket count. */
int osd_grad_buckets(const osd_config *cfg, int32_t *first, int32_t *last, int max_buckets);

/* ---- data-parallel gradient exchange over RCCL / xGMI ------------------------------
 * The reference is single-process; the slot these fill is between loss.backward() and clip_grad_norm_
 * (utils/train.py:239-244).  One communicator per process (one process per GPU).  RCCL is bound at run time
 * (dlopen): OSD_EUNSUPPORTED when no librccl.so can be found.
 *   osd_comm_unique_id   rank 0 draws the 128-byte rendezvous id (ncclGetUniqueId); the caller ships it to the
 *                        other ranks (the Python shim broadcasts it through torch.distributed's store)
 *   osd_comm_create      collective over all ranks (ncclCommInitRank) on HIP device `device`
 *   osd_allreduce_grads_begin  SUM all-reduce of flat_grad[start[b], end[b]) (element offsets) for b = 0..n_buckets-1
 *                        on the communicator's stream; bucket b waits for events[b] (the hipEvent_t array handed
 *                        to osd_train_loss_fwd_bwd), or -- events == NULL -- for everything queued on the
 *                        handle's stream.  Gradients are pre-scaled by 1/world through loss_scale.
 *   osd_allreduce_grads_end    the handle's stream waits for the collectives (then clip + AdamW may run) */
#define OSD_COMM_ID_BYTES 128
typedef struct osd_comm osd_comm;
int osd_comm_unique_id(void *id_out128);
int osd_comm_create(const void *id128, int rank, int world, int device, osd_comm **out);
int osd_comm_destroy(osd_comm *c);
int osd_allreduce_grads_begin(osd_handle *h, osd_comm *c, float *flat_grad, const int64_t *start,
                              const int64_t *end, void *const *events, int n_buckets);
int osd_allreduce_grads_end(osd_handle *h, osd_comm *c);

/* MixupAugmentation.__call__ (utils/train.py:108-120): out = lam*v + (1-lam)*v[perm]
 * for data[n][D], conditions[n][cond_dim], survival[n]; perm dev int64[n]. */
int osd_mixup(osd_handle *h, const float *data, const float *cond, const float *surv,
              const int64_t *perm, double lam, int64_t n, float *data_out, float *cond_out,
              float *surv_out);

/* clip_grad_norm_(max_norm) + AdamW.step (utils/train.py:242-244, 169-173) over flat
 * contiguous buffers of `numel` floats.  step is the 1-based count after increment.
 * grad_norm_out (dev float[1], may be NULL) receives the pre-clip global L2 norm.
 * max_norm <= 0 disables clipping.  Hyper-parameters are python floats (doubles): derived
 * scalars such as 1 - beta2 are formed in double and rounded to fp32 once, as torch does. */
int osd_clip_adamw_step(osd_handle *h, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                        int64_t numel, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double max_norm, int64_t step, float *grad_norm_out);

/* The same step without a model handle (any nn.Module's flat buffers, e.g. the cVAE): normsq_ws is
 * caller-owned device scratch of 256 doubles (no initial state needed: the global gradient norm is formed from one partial
 * sum per workgroup, added up in a fixed order -- deterministic, and independent of any previous call). */
int osd_nn_clip_adamw_step(void *stream, int device, double *normsq_ws, float *param, float *grad,
                           float *exp_avg, float *exp_avg_sq, int64_t numel, double lr, double beta1,
                           double beta2, double eps, double weight_decay, double max_norm, int64_t step,
                           float *grad_norm_out);

/* Both steps with an exponential moving average of the parameters kept in the same pass: after the AdamW update of an element,
 *   ema = ema + w * (param_new - ema),   w = (float)(1.0 - ema_decay)        (ema.lerp_(param, 1 - ema_decay), three fp32 roundings)
 * ema is a device float[numel] holding the running average (the caller initialises it, usually as a copy of param).  The library
 * knows nothing about warm-up: the caller passes each step's decay.  ema_decay 0 leaves ema == param, 1 leaves ema untouched.
 * OSD_EINVAL for a NULL ema and for ema_decay outside [0, 1] (checked before any device call).  param, grad, the moments and
 * grad_norm_out receive exactly what the plain step writes. */
int osd_clip_adamw_ema_step(osd_handle *h, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                            int64_t numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                            double max_norm, int64_t step, double ema_decay, float *grad_norm_out);
int osd_nn_clip_adamw_ema_step(void *stream, int device, double *normsq_ws, float *param, float *grad,
                               float *exp_avg, float *exp_avg_sq, float *ema, int64_t numel, double lr,
                               double beta1, double beta2, double eps, double weight_decay, double max_norm,
                               int64_t step, double ema_decay, float *grad_norm_out);

/* ---- the grouped step: fine-tuning from a pretrained model ----
 * The flat buffer is cut into n_groups sorted, non-empty, non-overlapping element ranges [begin, end) that together cover
 * [0, numel); at most OSD_MAX_PARAM_GROUPS of them.  Offsets are element offsets and need no alignment.  Each group scales the
 * learning rate (lr_scale) and the weight decay (wd_scale) and may pull its parameters toward `anchor` (l2sp, the L2-SP penalty of
 * Li et al. 2018, decoupled like the weight decay).  The per-group constants are formed in double and rounded once to float:
 *   decay_s = 1 - lr*lr_scale*weight_decay*wd_scale,   neg_step_size_s = -(lr*lr_scale / bc1),   pull_s = lr*lr_scale*l2sp.
 * Per element of a group with lr_scale > 0, in fp32 with one rounding per operation:
 *   g *= coef (when max_norm > 0);  p_old = p;  p = p*decay_s;  if (pull_s != 0) p = p - pull_s*(p_old - anchor);
 *   then the moments, the addcdiv and (ema != NULL) the lerp of the plain step.  With lr_scale = wd_scale = 1 and l2sp = 0 these are
 *   the plain step's operations in its order, and the result carries its bits.
 * A group with lr_scale == 0 is FROZEN: none of param, grad, exp_avg, exp_avg_sq, ema is written there, and its gradient is left out of
 * the norm by a select (a NaN or 1e30 there does not reach coef or grad_norm_out): clip_grad_norm_ over the parameters that have
 * gradients.  With no frozen group grad_norm_out carries the plain step's bits.  All groups frozen is legal: norm 0, nothing written.
 * No atomics, no state between calls; the same bits however a run of equal-setting elements is cut into groups.
 * ema and anchor are nullable device float[numel]; anchor is read only inside groups with pull_s != 0.  groups_host is host memory,
 * consumed before the call returns.  normsq_ws (the stream-taking variant): device scratch of OSD_GROUP_WS_DOUBLES doubles -- the
 * norm partials and room for the group table -- with no initial state required.
 * OSD_EINVAL, before any device call: a NULL buffer; n_groups outside [1, OSD_MAX_PARAM_GROUPS]; groups unsorted, empty, overlapping
 * or not covering [0, numel); a negative or non-finite scale; l2sp > 0 in some group with a NULL anchor; ema_decay outside [0, 1]
 * when ema is given.  The handle variant marks the packed weight copies stale, as the plain handle step does. */
#define OSD_MAX_PARAM_GROUPS 1024
#define OSD_GROUP_WS_DOUBLES 3328 /* 256 + 3 * OSD_MAX_PARAM_GROUPS */
typedef struct { int64_t begin, end; float lr_scale, wd_scale, l2sp; } osd_param_group;
int osd_group_adamw_step(osd_handle *h, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                         float *ema /*nullable*/, const float *anchor /*nullable*/, int64_t numel,
                         const osd_param_group *groups_host, int n_groups, double lr, double beta1, double beta2,
                         double eps, double weight_decay, double max_norm, int64_t step, double ema_decay,
                         float *grad_norm_out);
int osd_nn_group_adamw_step(void *stream, int device, double *normsq_ws, float *param, float *grad, float *exp_avg,
                            float *exp_avg_sq, float *ema /*nullable*/, const float *anchor /*nullable*/, int64_t numel,
                            const osd_param_group *groups_host, int n_groups, double lr, double beta1, double beta2,
                            double eps, double weight_decay, double max_norm, int64_t step, double ema_decay,
                            float *grad_norm_out);

/* ---- differentially private training (DP-SGD, Abadi et al. 2016) ----
 * A training call on n rows has loss L = (1/n) sum_r l_r, l_r = (1/D) w[t_r] sum_f rho(d_rf) (osd_set_loss, osd_set_prediction, dropout and
 * condition dropout as configured).  With g_r = grad l_r over ALL parameter tensors taken as one vector and s_r = |g_r|_2,
 *   c_r = min(1, C / (s_r + 1e-6)),     G = (1/n) sum_r c_r g_r.
 * osd_set_dp_clip(h, C) with C > 0 makes every later osd_train_loss_fwd_bwd call with gradients return G in `grads` (the loss stays the
 * unclipped L) and set OSD_TP_DP_CLIP; persistent like osd_set_loss; C = 0 clears it and restores the default launches bit for bit.
 * OSD_EINVAL for a negative or non-finite C.  No per-row gradient is formed: every layer is a Linear or a per-row GroupNorm, so s_r^2 is
 * a sum of row norms of buffers the backward pass already holds; one launch measures them, a second scales the rows of the buffers
 * that the weight-gradient, column-sum and time-table launches read, and those launches run last.
 * Such a call returns OSD_EUNSUPPORTED, with the reason in osd_last_error() and before any launch (no gradient buffer is touched), when
 * bucket events are requested or loss_scale != 1 (data parallel), constraint terms are configured (batch statistics: no per-row
 * gradient), an armed osd_train_batch_source has idx_b != NULL (mixup: one record in two rows), or a hidden width is not 256 / 512
 * (GroupNorm groups outside the fused backward).  It never returns unclipped gradients.  Calls without gradients are unaffected;
 * osd_denoiser_backward (a caller's own loss) returns OSD_EUNSUPPORTED while a bound is set.
 * Two limits of the guarantee built on this: the (epsilon, delta) account of the Python Trainer assumes Poisson sampling at rate B/N
 * while batches are shuffled fixed-size ones, and the noise below comes from Philox, which is not a cryptographically secure generator. */
int osd_set_dp_clip(osd_handle *h, double max_grad_norm);
/* s_r of the last clipped call's n rows into dst_dev (dev float[n]), asynchronously on the handle's stream.  OSD_ESTATE if there was
 * none, OSD_EINVAL for another n. */
int osd_dp_row_norms(osd_handle *h, float *dst_dev, int64_t n);
/* The AdamW step of osd_clip_adamw_step / ..._ema_step with Gaussian noise in place of the batch clip (which is off: the per-row clip
 * already bounds |G| <= C): the gradient element at flat position i becomes g + noise_std * z_i, is written back to grad, and goes
 * through AdamW; one launch, no norm pass.  DP-SGD's noise_std is sigma * C / n.  z_i is a Philox4x32-10 + Box-Muller normal: the four
 * values of positions 4q .. 4q + 3 come from the block at counter (q / 1024, q % 1024, step, 0x44504e00) under key `seed` -- the flat
 * buffer read as rows of 4 096 elements.  noise_std 0 adds nothing (and leaves grad unwritten).  There is no grad_norm_out.
 * OSD_EINVAL for a negative or non-finite noise_std and for step outside [1, 2^32). */
int osd_dp_adamw_step(osd_handle *h, float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t numel, double lr,
                      double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed, int64_t step);
int osd_nn_dp_adamw_step(void *stream, int device, float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t numel,
                         double lr, double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed,
                         int64_t step);
int osd_dp_adamw_ema_step(osd_handle *h, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *ema, int64_t numel,
                          double lr, double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed,
                          int64_t step, double ema_decay);
int osd_nn_dp_adamw_ema_step(void *stream, int device, float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                             int64_t numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                             double noise_std, uint64_t seed, int64_t step, double ema_decay);

/* Measurement aid for tools/dp_bench.py: the last clipped training call's row-norm launch (which = 0) or clip-factor launch (1) again, on
 * the buffers that call left in the workspace; which = 2 sets every clip factor to `fill` first (a launch skips rows whose factor is 1).
 * OSD_ESTATE if there was no such call, if any call has carved the training workspace since (another batch size may have re-allocated
 * it), or if that call read its conditions from the caller's tensor and not from the workspace (a batch source or condition dropout
 * puts them there).  The workspace no longer holds a step's values afterwards. */
int osd_dp_replay(osd_handle *h, int which, float fill);

/* Measurement aid for bench.py: per-launch HIP-event timing of one reverse step on n rows
 * (eager launches on the handle's stream, averaged over reps after one warm-up pass).
 * Entry 0 = input_proj, 1..2*n_blocks = the Linear+GroupNorm+SiLU halves in execution order,
 * last = output_proj+posterior.  flop_out = algorithmic GEMM FLOPs of each launch. */
int osd_profile_step(osd_handle *h, const float *cond, int64_t n, int reps, float *ms_out,
                     double *flop_out, int max_entries, int *n_entries);

/* ---- validation metrics on the device (utils/validation.py) ----------------
 * Stream/device based (no model handle), synchronous: results are host scalars. */
/* compute_mmd (utils/validation.py:273-298): RBF kernel, gamma <= 0 -> 1/D, means over all pairs
 * including the diagonal, sqrt(max(XX + YY - 2 XY, 0)).  X dev [n][D], Y dev [m][D]. */
int osd_val_mmd(void *stream, int device, const float *X, int64_t n, const float *Y, int64_t m, int D,
                double gamma, double *mmd_out);
/* One block of the above for row-sharded data (multi-GPU validation): sum_out = sum_{i<n, j<m} exp(-gamma |a_i - b_j|^2). */
int osd_val_rbf_sum(void *stream, int device, const float *A, int64_t n, const float *B, int64_t m, int D,
                    double gamma, double *sum_out);
/* For every row of Q dev [nq][D]: the nearest row of R dev [nr][D] in squared Euclidean distance, skipping row exclude[i]
 * (dev int32 [nq] or NULL; values outside [0, nr) exclude nothing).  idx_out dev int32 [nq]: the smallest index among the
 * minimisers of the fp32 expanded form; d2_out dev float [nq]: sum_k (Q[i][k] - R[idx][k])^2 recomputed directly.
 * No candidate: idx -1, d2 +inf.  Inputs must be finite.  Synchronous, like the other osd_val_* calls. */
int osd_val_nearest(void *stream, int device, const float *Q, int64_t nq, const float *R, int64_t nr, int D,
                    const int32_t *exclude, float *d2_out, int32_t *idx_out);
/* osd_val_nearest for the k nearest rows, 1 <= k <= 16 (OSD_EINVAL otherwise), in one pass over the nq x nr rectangle.
 * d2_out dev float [nq][k], idx_out dev int32 [nq][k]; workspace O(nq k + nr).  The k rows are the k smallest of the key
 * (float_bits(max(|r|^2 + |q|^2 - 2 r.q, 0)) << 32) | index, so ties of the fp32 expanded form go to the smaller index and the
 * result is a function of the inputs alone; their distances are recomputed directly as in osd_val_nearest (an exact copy is
 * 0.0f) and the k pairs of a query are then RE-SORTED by (recomputed distance, index) ascending: d2_out[i][k-1] is the largest of
 * the list, the row's k-th-neighbour radius.  Fewer than k candidates: the tail is idx -1, d2 +inf.  k = 1 returns
 * osd_val_nearest's outputs bit for bit.  exclude, the finite inputs and the synchronous return as in osd_val_nearest. */
int osd_val_knn(void *stream, int device, const float *Q, int64_t nq, const float *R, int64_t nr, int D, int k,
                const int32_t *exclude, float *d2_out, int32_t *idx_out);
/* Rows inside a radius, counted over the same rectangle without materialising it.  With d2(p, f) = max(|r_f|^2 + |q_p|^2 - 2 r_f.q_p, 0)
 * in fp32 (the expanded form: its rounding error scales with the squared norms, so a row AT a radius may fall on either side):
 *   in_ref_out[p]   = #{f : d2(p, f) <= r2_ref[f]},    r2_ref dev float [nr]: a radius per reference row
 *   in_query_out[p] = #{f : d2(p, f) <= r2_query[p]},  r2_query dev float [nq]: a radius per query row
 * both dev int32 [nq], overwritten.  Either radius / output pair may be NULL (a radius without its output, or neither pair, is
 * OSD_EINVAL).  Radii are squared distances; +inf holds every row, a negative or NaN radius none.  Exact integer counts,
 * independent of the order of execution.  Inputs must be finite.  Synchronous. */
int osd_val_ball_counts(void *stream, int device, const float *Q, int64_t nq, const float *R, int64_t nr, int D,
                        const float *r2_ref, const float *r2_query, int32_t *in_ref_out, int32_t *in_query_out);
/* scipy.stats.ks_2samp as used at utils/validation.py:238-245, for features 0..nf-1 of real dev [n1][ld]
 * and synth dev [n2][ld]: exact integer extremes of cnt(real<=v)*n2 - cnt(synth<=v)*n1 over all sample
 * points v; the statistic is max(dmax, -dmin, 0) / (n1*n2) (p-values follow on the host). */
int osd_val_ks_extremes(void *stream, int device, const float *real, int64_t n1, const float *synth,
                        int64_t n2, int ld, int nf, int64_t *dmax_out, int64_t *dmin_out);
/* Per-feature two-sample statistics over ALL D columns of real dev [n1][ld_real] and synth dev [n2][ld_synth] (fp32, row-major,
 * any base alignment; a column-slice view is read in place).  With a the real column sorted ascending (n1 values) and b the
 * synthetic one (n2 values), per feature into HOST arrays of D entries:
 *   ks_dmax, ks_dmin  the extremes over all pooled sample points v of #{a <= v} n2 - #{b <= v} n1: exact integers, the quantity
 *                     osd_val_ks_extremes returns; KS = max(dmax, -dmin) / (n1 n2)
 *   w1                the Wasserstein-1 distance by quantile coupling, (1 / (n1 n2)) sum |a_i - b_j| w_ij with the integer weights
 *                     w_ij = min((i + 1) n2, (j + 1) n1) - max(i n2, j n1) > 0: differences, products and the sum in double, in an
 *                     order fixed by (n1, n2) -- the same bits on every call and at every chunk_cols
 *   below, above      #{b < a_0} and #{b > a_(n1 - 1)}: synthetic values outside the real column's range
 * The columns are transposed, sorted (the segmented radix sort of osd_val_ks_extremes) and compared chunk_cols at a time, so the
 * workspace does not grow with D; chunk_cols = 0 picks osd_val_marginals_auto_chunk(n1, n2, D).  OSD_EINVAL for a NULL pointer,
 * n1, n2 or D below 1, an ld below D, a negative chunk_cols, more than 2 * 10^9 rows, or n1 * n2 > 2^53 (up to there every weight
 * and KS integer converts to double exactly).  Inputs must be finite.  Synchronous. */
int osd_val_marginals(void *stream, int device, const float *real, int64_t n1, int ld_real, const float *synth,
                      int64_t n2, int ld_synth, int D, int chunk_cols, int64_t *ks_dmax, int64_t *ks_dmin, double *w1,
                      int64_t *below, int64_t *above);
/* The same call, and into phase_ms[3] (host) the device milliseconds of its three phases summed over the chunks: the transposing
 * gather, the sort, the statistics pass (tools/marginal_bench.py). */
int osd_val_marginals_timed(void *stream, int device, const float *real, int64_t n1, int ld_real, const float *synth,
                            int64_t n2, int ld_synth, int D, int chunk_cols, int64_t *ks_dmax, int64_t *ks_dmin,
                            double *w1, int64_t *below, int64_t *above, double *phase_ms);
/* The columns per chunk that chunk_cols = 0 stands for (a negative OSD_E* code on a bad argument): the transposed and the sorted
 * buffer of both cohorts, 8 (n1 + n2) bytes per column, together within 256 MiB, in whole multiples of 64 columns from 64 up. */
int osd_val_marginals_auto_chunk(int64_t n1, int64_t n2, int D);
/* Per-feature two-GROUP rank statistics inside ONE cohort (csrc/diffexp.hip): X dev float [rows][ld] (fp32,
 * row-major, any base alignment, any ld >= D; a column-slice view is read in place, once), labels dev int32 [rows]: 1 a case, 0 a
 * control, any other value a row that is ignored.  With a the feature's case values sorted ascending (na of them), b its control
 * values (nb of them) and c its centre (center: dev float [D], or NULL for 0), per feature into HOST arrays:
 *   u2      int64 [D]      sum_i (#{b < a_i} + #{b <= a_i}): exactly twice the Mann-Whitney U of the cases over the controls with ties
 *                          counted 1/2 -- the per-feature AUC is u2 / (2 na nb)
 *   ties    int64 [D]      sum over the distinct values v of the pooled column of t_v^3 - t_v, t_v the number of pooled values equal
 *                          to v: the tie correction of the normal approximation (-0.0 and +0.0 are one value)
 *   sum, sumsq  double [2][D]   sum (x - c) and sum (x - c)^2 over the cases ([0][j]) and over the controls ([1][j]): the difference
 *                          and the square in double, summed over the SORTED values in an order fixed by (na, nb)
 *   na, nb  int64 [1]      the group sizes (written before the group checks below)
 * Integer results are exact.  No atomics, and the partition of the work depends on (na, nb) alone: the same bits on every call, at
 * every chunk_cols and for every permutation of the rows.  The columns are gathered by label, sorted (the segmented radix sort of
 * osd_val_ks_extremes) and compared chunk_cols at a time; chunk_cols = 0 picks osd_val_marginals_auto_chunk(na, nb, D).
 * OSD_EINVAL for a NULL pointer (center excepted), rows or D below 1, an ld below D, a negative chunk_cols, more than 2 * 10^9 rows,
 * na == 0 or nb == 0, or na + nb > 2^20 (up to there ties stays below 2^60).  Inputs must be finite.  Synchronous. */
int osd_val_group_ranks(void *stream, int device, const float *X, int64_t rows, int ld, int D, const int32_t *labels,
                        const float *center, int chunk_cols, int64_t *u2, int64_t *ties, double *sum, double *sumsq,
                        int64_t *na, int64_t *nb);
/* The same call, and into phase_ms[3] (host) the device milliseconds of its three phases summed over the chunks: the
 * label-partitioned gather, the sort, the statistics pass (tools/diffexp_bench.py). */
int osd_val_group_ranks_timed(void *stream, int device, const float *X, int64_t rows, int ld, int D, const int32_t *labels,
                              const float *center, int chunk_cols, int64_t *u2, int64_t *ties, double *sum, double *sumsq,
                              int64_t *na, int64_t *nb, double *phase_ms);
/* The permutation null of preranked gene-set enrichment analysis (csrc/gsea.hip).  All arrays are HOST
 * arrays.  weights_host double [D]: the weight of every position of the ranked gene list (|statistic| ** weight; all ones is the
 * classic Kolmogorov-Smirnov form).  Set s holds the ranked positions set_positions_host[set_offsets_host[s] ..
 * set_offsets_host[s + 1]) (set_offsets_host int32 [S + 1], starting at 0), in any order, k of them.  With its hit positions
 * ascending h_0 < ... < h_{k-1}, C_j = w[h_0] + ... + w[h_j] added one after another in double (C_{-1} = 0) and NR = C_{k-1}:
 *   up_j = C_j / NR - (h_j - j) / (D - k)        dn_j = C_{j-1} / NR - (h_j - j) / (D - k)
 * (two divisions and one subtraction each; with NR == 0 the ratios are (j + 1) / k and j / k), and
 *   es_pos_host  double [permutations + 1][S]   max_j up_j
 *   es_neg_host  double [permutations + 1][S]   min_j dn_j
 *   lead_host    int32 [S][2]                   row 0 only: the first j that attains the maximum, the first that attains the minimum
 * Row 0 takes the positions as they are.  Row p >= 1 moves position i to rho_p(i), the rank of the pair (key_p(i), i) among all D
 * such pairs -- key_p(i) is word 0 of the Philox4x32-10 block at counter (i, p, 0, 0x47534500) under the key (seed) -- so every set
 * sees the same permutation of the gene labels and overlapping sets stay correlated.  The permutations go through perm_chunk at a
 * time (0: as many as fill 64 MiB of workspace, which therefore does not grow with `permutations`); no atomics: the same bits at
 * every perm_chunk and on every call, and equal to the float64 restatement of the definition bit for bit.  The ranks come from a
 * sort of the keys in LDS; with OSD_GSEA_RANKS=count in the environment they are counted instead (slower, the same bits).
 * OSD_EINVAL for a NULL pointer, D outside [2, 32768], S < 1, a set with k < 1, k > 1024 or k >= D, a position outside [0, D) or
 * repeated inside a set, a weight that is negative, not finite or above 1e100, permutations < 0 or perm_chunk < 0.  Synchronous. */
int osd_val_gsea(void *stream, int device, const double *weights_host, int D, const int32_t *set_offsets_host,
                 const int32_t *set_positions_host, int S, int permutations, uint64_t seed, int perm_chunk, double *es_pos_host,
                 double *es_neg_host, int32_t *lead_host);
/* The same call, and into phase_ms3[3] (host) the device milliseconds of its three phases summed over the chunks: keys and ranks,
 * the hit sort, the running-sum scan (tools/gsea_bench.py). */
int osd_val_gsea_timed(void *stream, int device, const double *weights_host, int D, const int32_t *set_offsets_host,
                       const int32_t *set_positions_host, int S, int permutations, uint64_t seed, int perm_chunk, double *es_pos_host,
                       double *es_neg_host, int32_t *lead_host, float *phase_ms3);
/* Per-patient pathway scores (csrc/pathway.hip).  X dev float [rows][ld] (fp32, row-major, any base
 * alignment, any ld >= D; a column-slice view is read in place, once).  Set s holds the m distinct columns set_members_host[
 * set_offsets_host[s] .. set_offsets_host[s + 1]) (HOST arrays, set_offsets_host int32 [S + 1] starting at 0).  Every score is a
 * function of its row alone, into out dev double [rows][S]:
 *   method 0 (mean)    (sum_j (x_j - c_j) s_j) / m          c = center, s = scale: dev float [D], or NULL for 0 and for 1
 *   method 1 (zscore)  (sum_j (x_j - c_j) s_j) / sqrt(m)    the combined z-score of Lee et al. 2008 with c the cohort's mean and s 1 / sd
 *   method 2 (ssgsea)  sum_j r_j T[2 r_j] / sum_j T[2 r_j] - (D (D + 1) / 2 - sum_j r_j) / (D - m)
 * the differences, products and sums in double.  r_g is the ascending mid-rank of x_g among the row's D values (1 ... D, ties
 * averaged, -0.0 and +0.0 equal, +-inf ordered as values): 2 r_g = #{x < x_g} + #{x <= x_g} + 1 is an exact integer, and
 * rank_table_host double [2 D + 1] (HOST; method 2 only, else it may be NULL) holds T[k] = (k / 2)^alpha -- the enrichment score of
 * Barbie et al. 2009 as the sum over the walk's positions of P_hit - P_miss.  A row that holds a NaN gets NaN for all its ssgsea
 * scores; the linear methods propagate NaN by IEEE arithmetic.  row_chunk rows go into one launch (0: up to 2^20).  No atomics, a
 * fixed order of every sum: the same bits on every call, at every row_chunk and from the _timed twin; a permutation of the rows
 * permutes the outputs and a set listed twice gets the same bits twice.
 * OSD_EINVAL for a NULL pointer (center and scale excepted), a method outside 0 .. 2, D outside [2, 32768], rows < 1, ld < D, S < 1,
 * row_chunk < 0, a set with m < 1, m > 1024 or m >= D, a member outside [0, D) or repeated inside a set.  Synchronous. */
int osd_val_pathway_scores(void *stream, int device, const float *X, int64_t rows, int ld, int D, int method, const float *center,
                           const float *scale, const int32_t *set_offsets_host, const int32_t *set_members_host, int S,
                           const double *rank_table_host, int row_chunk, double *out);
/* The same call, and into phase_ms2[2] (host) the device milliseconds of its two phases: the staging of the tables, the scoring
 * launches (tools/pathway_bench.py). */
int osd_val_pathway_scores_timed(void *stream, int device, const float *X, int64_t rows, int ld, int D, int method, const float *center,
                                 const float *scale, const int32_t *set_offsets_host, const int32_t *set_members_host, int S,
                                 const double *rank_table_host, int row_chunk, double *out, float *phase_ms2);
/* A generated pathway block against the scores of the same patients' expression (csrc/pathway.hip): scores dev double [rows][S],
 * block dev float [rows][ld_b] (its first S columns are used), mu_host and isd_host HOST double [S].  With z = (score - mu) * isd
 * and g the block's value, over the rows where both are finite, into sums_host HOST double [S][6] per pathway
 *   sum z, sum g, sum z^2, sum g^2, sum z g, sum (g - z)^2
 * and into used_host HOST int64 [S] the number of those rows (rows - used_host[s] were left out).  Sums in double, no atomics, in
 * an order fixed by `rows`: the same bits on every call.
 * OSD_EINVAL for a NULL pointer, rows < 1, S outside [1, 65535] or ld_b < S.  Synchronous. */
int osd_val_pathway_agreement(void *stream, int device, const double *scores, int64_t rows, int S, const float *block, int ld_b,
                              const double *mu_host, const double *isd_host, double *sums_host, int64_t *used_host);
/* Mean of the strict upper triangle of the Pearson matrix of data[:, cols] (utils/validation.py:156-161);
 * cols: host array of g column indices, 2 <= g <= 512. */
int osd_val_mean_offdiag_corr(void *stream, int device, const float *data, int64_t rows, int ld,
                              const int32_t *cols_host, int g, double *out);
/* Column sums (double) of data[:, :cols] -- the mutation frequencies of utils/validation.py:45-46 are sums / rows. */
int osd_val_column_sums(void *stream, int device, const float *x, int64_t rows, int ld, int cols,
                        double *sums_host);
/* Raw Gram matrix of up to 64 selected columns: gram_host[i*g + j] = sum_r x[r][c_i] * x[r][c_j].  For 0/1 mutation
 * columns these are the exact joint counts behind the 2x2 contingency tables of utils/validation.py:98-111 and
 * the both-mutated counts of :75-78. */
int osd_val_gram(void *stream, int device, const float *x, int64_t rows, int ld, const int32_t *cols_host,
                 int g, double *gram_host);
/* The two passes of osd_val_mean_offdiag_corr as partial sums over a row shard (all-reduce between them):
 * per selected column sum and sum of squares; then S = sum_rows (sum_g (x - mu_g) * isd_g)^2. */
int osd_val_col_moments(void *stream, int device, const float *data, int64_t rows, int ld,
                        const int32_t *cols_host, int g, double *sum_host, double *sumsq_host);
int osd_val_rowz_sq(void *stream, int device, const float *data, int64_t rows, int ld,
                    const int32_t *cols_host, int g, const double *mu_host, const double *isd_host,
                    double *S_host);
/* Pearson correlation of two strided device columns (Series.corr at utils/validation.py:205); the five raw
 * sums (sum a, sum b, sum a^2, sum b^2, sum ab) of a row shard. */
int osd_val_pearson_sums(void *stream, int device, const float *a, int lda, const float *b, int ldb,
                         int64_t rows, double *out5_host);
int osd_val_pearson(void *stream, int device, const float *a, int lda, const float *b, int ldb,
                    int64_t rows, double *out);
/* Centred Gram matrix of a whole cohort (csrc/corr.hip):
 *   G[i][j] = sum_r (X[r][i] - c[i]) * (X[r][j] - c[j]),   i, j < D.
 * X dev float [rows][ld], the first D columns used (any rows >= 1, D >= 1, ld >= D; an X whose base or ld does not suit 16-byte
 * staging is first copied to a padded device buffer of rows * roundup(D, 4) floats); center_host: host float [D]; G_dev: DEVICE
 * double [D][D], overwritten, exactly symmetric.  Differences and products are fp32 (the fp32 MFMA), accumulated in fp32 over runs of
 * at most OSD_COV_SLAB_ROWS rows; every run is folded into double sums owned by one work item (128 x 128 tile on or above the
 * diagonal x row slice), the slices of a tile are summed in a fixed order: no floating-point atomics, the same inputs give the
 * same bits.  The number of row slices follows the tile count and the CU count, never rows: workspace O(slices * D^2).
 * Inputs must be finite.  D <= 32768.  Synchronous. */
#define OSD_COV_SLAB_ROWS 256
int osd_val_centered_gram(void *stream, int device, const float *X, int64_t rows, int ld, int D,
                          const float *center_host, double *G_dev);
/* Two Gram matrices of osd_val_centered_gram (dev double [D][D], real and synthetic cohort) compared as correlation matrices
 * without storing either: r = G[i][j] / sqrt(G[i][i] * G[j][j]) in double, delta = r_synth - r_real, over the pairs i < j of
 * columns that are not constant (G[i][i] <= 0 in either matrix).  bounds_host: host int32 [n_blocks + 1], 0 = b_0 < b_1 < ... <
 * b_n_blocks = D (OSD_EINVAL otherwise) -- column blocks.  out_host: host double [1 + OSD_CORR_STATS * n_blocks (n_blocks + 1) / 2]:
 * out[0] the number of constant columns, then for every block pair a <= b in row-major order (0,0), (0,1), ..., (1,1), ... over the
 * pairs with i in block a and j in block b:
 *   [0] pairs  [1] sum |delta|  [2] sum delta^2  [3] max |delta|  [4] strong pairs: |r_real| >= strong
 *   [5] strong pairs with sign(r_synth) == sign(r_real)  [6] sum |delta| over the strong pairs.
 * Counts and the maximum are exact; the sums are double atomics (last-bit freedom).  Synchronous. */
#define OSD_CORR_STATS 7
int osd_val_corr_compare(void *stream, int device, const double *G_real, const double *G_synth, int D,
                         const int32_t *bounds_host, int n_blocks, double strong, double *out_host);
/* Loss, gradient and scores of K regularised-linear-model heads over a cohort, in one read of X (csrc/glm.hip; DESIGN.md section
 * 3.22).  With u_i = (x_i - center) * scale over the first D columns, z_ik = W_k[:D] . u_i + W_k[D] and a_i the row weight:
 *   loss_host[k]  = sum_i a_i l_k(y_ik, z_ik)            l = softplus(z) - y z (OSD_GLM_LOGISTIC), (z - y)^2 / 2 (OSD_GLM_SQUARED)
 *   grad_dev[k]   = sum_i a_i dl/dz (u_i, 1)              DEVICE double [K][D + 1], bias last, overwritten; a column with scale 0
 *                                                         is dropped (gradient exactly 0)
 *   score_dev     = z_ik                                  dev float [rows][lds]
 * SUMS, not means, and no penalty: the results of several calls (two cohorts, row shards, row chunks) add up; the host applies 1 / n
 * and the L2 term.  X dev float [rows][ld] (any base address, any ld >= D: a 16-byte aligned base with ld % 4 == 0 and
 * ld >= roundup(D, 4) is read 16 bytes per lane, everything else by dwords in place -- never through a copy); center, scale: dev
 * float [D]; Y: dev float [rows][ldy], the first K columns (logistic targets are used as given: soft labels are legal); row_weight:
 * dev float [rows] or NULL (= 1); W: dev float [K][D + 1]; kind_host: host int32 [K].  grad_dev == NULL: the predictor -- scores
 * (and the loss, if asked for) with the bits of the full call and no column accumulation.  loss_host and score_dev may be NULL, Y
 * too if neither loss nor gradient is asked for; at least one output.
 * Arithmetic: x - center, the products and the dot are fp32 (the kernel multiplies W by scale once and applies the gradient's factor
 * scale in double); the logistic loss is max(z, 0) - y z + log1p(exp(-|z|)) and the sigmoid is finite for every finite z.  The
 * gradient is accumulated in fp32 over runs of at most OSD_GLM_RUN_ROWS rows per work item (a contiguous block of rows), every run
 * is folded into the item's double sums, and the items are added in a fixed order; the loss is summed in double from fp32 row
 * terms the same way.  No floating-point atomics: the same inputs give the same bits, and the partition into items depends on
 * (rows, D, K) alone.  Inputs must be finite.  1 <= K <= 4, rows >= 1, 1 <= D <= 8192 (OSD_EINVAL otherwise).  Synchronous. */
#define OSD_GLM_LOGISTIC 0
#define OSD_GLM_SQUARED  1
#define OSD_GLM_RUN_ROWS 128
int osd_val_glm_eval(void *stream, int device, const float *X, int64_t rows, int ld, int D,
                     const float *center, const float *scale, const float *Y, int ldy, const float *row_weight,
                     const float *W, int K, const int32_t *kind_host, double *loss_host, double *grad_dev,
                     float *score_dev, int lds);
/* Per column of the first D: sum_r (X[r][j] - center[j]) and sum_r (X[r][j] - center[j])^2 in double, one streaming pass,
 * fixed summation order (same inputs, same bits).  center: dev float [D] or NULL (= 0); sum_host, sumsq_host: host double [D].
 * Partial sums of row shards about one common centre add up; mean and variance follow on the host.  Synchronous. */
int osd_val_col_centered_moments(void *stream, int device, const float *X, int64_t rows, int ld, int D,
                                 const float *center, double *sum_host, double *sumsq_host);
/* Per-label column sums of a cohort, in one read of X (csrc/cluster.hip): the update half of a Lloyd
 * iteration and the per-subtype mean of any matrix.  Over the rows r with labels[r] == k:
 *   sums_dev[k][c]     = sum_r X[r][c]          DEVICE double [K][D], overwritten
 *   counts_dev[k]      = the number of such rows DEVICE int64 [K], exact
 *   value_sums_dev[k]  = sum_r value[r]          DEVICE double [K]; value: dev float [rows]; both NULL when not wanted (one
 *                                                without the other is OSD_EINVAL)
 * X dev float [rows][ld] (any base address, any ld >= D, read by dwords in place -- never through a copy); labels: dev int32
 * [rows]; a row whose label lies outside [0, K) -- the -1 of osd_val_nearest included -- contributes to nothing.
 * Arithmetic: every addition is a double addition of a converted float, so a sum is exact up to 2^-53 per add whatever the
 * partition (and exact on integer data).  A work item is a block of rows times 64 columns with its own double accumulators, added
 * in row order; the items' sums are added in a fixed order.  No floating-point atomics: the same inputs give the same bits, and
 * the partition depends on (rows, D, K) alone.  rows >= 1, 1 <= D <= 8192, 1 <= K <= 64 (OSD_EINVAL otherwise).  Synchronous. */
int osd_val_label_sums(void *stream, int device, const float *X, int64_t rows, int ld, int D,
                       const int32_t *labels, int K, const float *value,
                       double *sums_dev, int64_t *counts_dev, double *value_sums_dev);
/* Cox proportional hazards over a cohort with follow-up times t_i and event flags delta_i in {0, 1} (csrc/cox.hip; DESIGN.md section
 * 3.26).  A plan holds what depends on (t, delta) alone and is made once per fit, on the host: the stable descending-time order of
 * the rows, the first and the last position of every row's tie group (equal times) and the flags in that order, uploaded to
 * `device` on `stream`; every later osd_val_cox_eval of the plan runs on that device and stream.  time_host, event_host: HOST
 * double [rows].  OSD_EINVAL, checked on the host before any device call: a non-finite time, a flag other than 0 or 1, rows < 1 or
 * rows >= 2^31.  The library makes every index the kernels follow, and osd_val_cox_eval refuses another row count than the plan's:
 * nothing a caller passes later can become an out-of-range index.  osd_val_cox_plan_destroy(NULL) is OSD_OK. */
int osd_val_cox_plan_create(int device, void *stream, const double *time_host, const double *event_host, int64_t rows,
                            void **plan);
int osd_val_cox_plan_destroy(void *plan);
/* Loss, gradient and scores of the Breslow partial likelihood.  With u_i = (x_i - center) * scale over the first D columns,
 * eta_i = w . u_i (no intercept: the partial likelihood has none), m = max eta and e_i = exp(eta_i - m):
 *   S_i        = sum_{k: t_k >= t_i} e_k                              the risk set, tied times included (Breslow)
 *   *loss_host = -sum_i delta_i (eta_i - m - log S_i)                 HOST double, a SUM over the rows, no penalty
 *   grad_dev   = sum_j r_j u_j,  r_j = -delta_j + e_j sum_{i: delta_i = 1, t_i <= t_j} 1 / S_i      DEVICE double [D], overwritten;
 *                                                                     a column with scale 0 is dropped (gradient exactly 0)
 *   score_dev  = eta_i                                                dev float [rows]
 * X dev float [rows][ld] with the layouts and the two load paths of osd_val_glm_eval (any base address, any ld >= D, never through
 * a copy); center, scale, w: dev float [D]; rows must be the plan's.  Any of the three outputs may be NULL, not all: scores alone
 * read X once and nothing else; a loss without a gradient skips the second read.
 * A call is two reads of X with 1-D work between them.  (a) eta in fp32 with osd_val_glm_eval's arithmetic -- x - center,
 * w' = w * scale, the same summation order -- so a score has the bits that call gives for one head with the same weights and a
 * zero bias.  (b) in double and in a fixed order: the maximum, exp, the prefix sums in descending-time order read at the end of each
 * tie group, the loss terms, the suffix sums of delta / S read at the start of each tie group, and r, which is rounded to fp32.  A
 * scan is block sums, a scan of the sums by one workgroup, and an apply pass, as separate launches: no workgroup waits for another
 * inside a kernel.  (c) the gradient, accumulated in fp32 over runs of at most OSD_GLM_RUN_ROWS rows per work item, every run folded
 * into the item's double sums, the items added in a fixed order and the factor scale applied once, in double.  No floating-point
 * atomics: the same inputs give the same bits, and the partition depends on (rows, D) and the load path alone.
 * Inputs must be finite.  A score range wider than exp can hold (eta - m below about -745) underflows e to 0; where that empties the
 * risk set of an event, S = 0 and the loss is not finite (+inf or NaN) -- a line search rejects such a step, as utility.fit_glm's
 * does.  All censored: loss 0 and gradient 0 exactly.  rows >= 1, 1 <= D <= 8192, ld >= D (OSD_EINVAL otherwise, checked on the
 * host before any device call).  Synchronous; uses a grow-only per-device workspace held for the length of the call. */
int osd_val_cox_eval(void *plan, const float *X, int64_t rows, int ld, int D, const float *center, const float *scale,
                     const float *w, double *loss_host, double *grad_dev, float *score_dev);
/* The univariate Cox screen: one model per column, all columns in one call (csrc/cox_score.hip).  For every
 * column c on its own, everything in double, with u_ic = ((double) x_ic - center_c) * scale_c, k_c = |beta_c| R_c (R_c = bound_dev[c],
 * a caller's bound R_c >= max_i |u_ic|; k_c = 0 without bound_dev) and e_ic = exp(beta_c u_ic - k_c) <= 1; over the positions p of
 * the plan's descending-time order, the risk set of p being every position up to the END of p's tie group (Breslow) and A0, A1, A2
 * the sums of e, e u, e u^2 over it:
 *   loglik_dev[c] = sum_p delta_p (beta_c u_pc - k_c - log A0)       the partial log-likelihood (k_c cancels: a shift of the exponent)
 *   score_dev[c]  = sum_p delta_p (u_pc - A1 / A0)                   its derivative in beta_c
 *   info_dev[c]   = sum_p delta_p (A2 / A0 - (A1 / A0)^2)            minus its second derivative
 *   absmax_dev[c] = max_i |u_ic|                                     exact (a maximum of doubles); NULL: not wanted
 * beta_dev NULL means beta = 0 and takes a path without exp: e = 1 and A0 is the risk set's size, an integer.  At beta = 0 score_dev is
 * minus the gradient osd_val_cox_eval gives at w = 0, and score^2 / info the log-rank chi-square of the column.
 * X dev float [rows][ld] with the layouts and the two load paths of osd_val_glm_eval (any base address, any ld >= D, never through a
 * copy); center, scale: dev float [D]; beta_dev, bound_dev, the outputs: dev double [D]; rows must be the plan's.
 * A call reads X twice, rows gathered by the plan's order.  A work item is a block of OSD_COXS_ROWS consecutive positions times a
 * slab of 256 columns; a lane owns four columns of the slab and walks the block's rows in position order.  Pass 1 writes every item's
 * totals of e, e u, e u^2 (and the block's max |u|); one launch turns the totals into per-column exclusive prefixes over the blocks;
 * pass 2 re-reads X, carries the running sums from the prefix, adds delta_p (beta u - k) and delta_p u at every position and, at
 * every position that ends a tie group holding d > 0 events, d log A0, d A1 / A0 and d (A2 / A0 - (A1 / A0)^2); a last launch adds
 * the items' partial results in block order.  No floating-point atomics, no workgroup waits for another inside a kernel, every sum
 * has one fixed order: the same inputs give the same bits, the partition depends on (rows, D) and the load path alone, and the
 * arithmetic of one column depends neither on the other columns of the call nor on the load path.
 * A column with scale 0 is dropped: its three outputs are exactly 0 (absmax too).  All censored: exact zeros.  Inputs must be finite.
 * Without a bound, or with one smaller than max |u|, beta u - k can pass what exp holds; and with a valid bound the risk set of an
 * event whose every beta u - k lies below about -745 sums to A0 = 0: the column's outputs are then not finite (inf or NaN), that
 * column's alone -- survival.univariate_cox clamps |beta| R so that this cannot happen, and marks a non-finite column failed.
 * rows >= 1, 1 <= D <= 8192, ld >= D, loglik_dev, score_dev and info_dev all given (OSD_EINVAL otherwise, checked on the host
 * before any device call).  Synchronous; uses a grow-only per-device workspace held for the length of the call. */
#define OSD_COXS_ROWS 128
int osd_val_cox_score(void *plan, const float *X, int64_t rows, int ld, int D, const float *center, const float *scale,
                      const double *beta_dev, const double *bound_dev, double *loglik_dev, double *score_dev, double *info_dev,
                      double *absmax_dev);
/* The two skinny products of a block subspace iteration (csrc/pca.hip): the top principal directions of a
 * cohort without its D x D Gram matrix.  With u_rc = ((double) x_rc - center_c) * scale_c (scale NULL: 1), everything after the load
 * in double:
 *   osd_val_pca_project      Z_dev[r][j] = sum_c u_rc V[c][j]     DEVICE double [rows][l], overwritten
 *                            norm2_dev[r] = sum_c u_rc^2          DEVICE double [rows]; NULL: not wanted
 *   osd_val_pca_backproject  W_dev[c][j] = sum_r u_rc Z[r][j]     DEVICE double [D][l], overwritten
 * X dev float [rows][ld] with the layouts and the two load paths of osd_val_glm_eval (any base address, any ld >= D, a column-slice
 * view is read in place, never through a copy); center, scale: dev double [D]; V: dev double [D][l]; Z: dev double [rows][l].
 * One iteration of the subspace method is one call of each, so X is read twice.  A work item is a block of rows times a slab of
 * columns, one wavefront: project gives a lane one of 64 rows and adds its terms in column order, the slabs are then added in slab
 * order; backproject gives a lane two columns and adds the block's rows in row order, the blocks are then added in a fixed order.
 * Vector FMAs in double; the small matrix is read through wave-uniform addresses.  No floating-point atomics, no workgroup waits
 * for another: the same inputs give the same bits, and the partition depends on (rows, D, l) and the load path alone.  A column with
 * scale 0 contributes nothing.  Integer data within 2^53 give exact integers.  Inputs must be finite.
 * 1 <= l <= OSD_PCA_MAX_DIRS, l <= D <= 32768, ld >= D, 1 <= rows < 2^31, no NULL pointer but scale and norm2_dev (OSD_EINVAL
 * otherwise, checked on the host before any launch).  Synchronous; uses a grow-only per-device workspace held for the length of the
 * call. */
#define OSD_PCA_MAX_DIRS 32
int osd_val_pca_project(void *stream, int device, const float *X, int64_t rows, int ld, int D, const double *center,
                        const double *scale, const double *V, int l, double *Z_dev, double *norm2_dev);
int osd_val_pca_backproject(void *stream, int device, const float *X, int64_t rows, int ld, int D, const double *center,
                            const double *scale, const double *Z_dev, int l, double *W_dev);
/* Harrell's concordance counts of a risk score, exact. Over the ordered pairs (i, j) with event[i] != 0 and time[i] < time[j]
 * (strict: equal times are not comparable), counts_host (HOST int64 [4]) receives
 *   [0] the comparable pairs   [1] those with risk[i] > risk[j] (concordant)   [2] risk[i] < risk[j]   [3] risk[i] == risk[j]
 * and C = ([1] + [3] / 2) / [0].  time_dev, event_dev, risk_dev: dev float [n]; comparisons are those of the fp32 values.  A lane
 * owns one i of a tile of OSD_CONC_I_TILE and meets every j once, OSD_CONC_J_CHUNK of them at a time through LDS; its 32-bit
 * counters are added in 64 bits through the wave and the workgroup's own slab, and the slabs on the host: integer sums, so the
 * result does not depend on any order, and nothing overflows below n = 2^31.  1 <= n < 2^31 (OSD_EINVAL otherwise, checked on the
 * host before any device call).  Synchronous. */
#define OSD_CONC_I_TILE  256
#define OSD_CONC_J_CHUNK 1024
int osd_val_concordance(void *stream, int device, const float *time_dev, const float *event_dev, const float *risk_dev,
                        int64_t n, int64_t *counts_host);

/* ---- feature transforms (csrc/transform.hip) ------------------------------
 * dst[r][f] = map_f(src[r][f]) over the first D columns of `rows` rows; inverse != 0 applies the inverse maps.  kind_dev[f]:
 *   OSD_XF_IDENTITY         copy
 *   OSD_XF_STANDARD         forward (x - center[f]) / scale[f]; inverse z * scale[f] + center[f], two roundings (no fma)
 *   OSD_XF_QUANTILE_NORMAL  a monotone piecewise-linear map between the column's knots k = knots_dev[f][0..Q-1] (fp32, non-decreasing)
 *                           and the levels zl = levels_dev[0..Q-1] (fp32, strictly increasing, shared by all columns).  NaN -> NaN.
 *     forward(x): lb = #{k < x}, ub = #{k <= x};  ub == 0 -> zl[0];  lb == Q -> zl[Q-1];  ub > lb (x equals the knots lb..ub-1, a tie
 *                 plateau) -> the mid-rank level 0.5 * (zl[(lb+ub-1)>>1] + zl[(lb+ub)>>1]);  else j = lb - 1,
 *                 t = (x - k[j]) / (k[j+1] - k[j]),  z = zl[j] + t * (zl[j+1] - zl[j])
 *     inverse(z): z <= zl[0] -> k[0];  z >= zl[Q-1] -> k[Q-1];  else j with zl[j] <= z < zl[j+1],
 *                 t = (z - zl[j]) / (zl[j+1] - zl[j]),  x = k[j] + t * (k[j+1] - k[j])
 *   Every operation is an fp32 operation in the order written; an interpolated result is then clamped to its bracket [zl[j],
 *   zl[j+1]] or [k[j], k[j+1]] (a + fl(b - a) can pass b by an ulp), so an inverse value lies inside [k[0], k[Q-1]] bit for bit and a
 *   plateau's whole z interval returns the tied value exactly.
 * src, dst: dev float [rows][ld]; src == dst (in place) is allowed, any other overlap is not; ld >= D: a column slice of a wider
 * matrix, whose other columns are neither read nor written.  knots_dev: dev float [D][Q] (rows of columns that are not quantile
 * columns are not read); center_dev, scale_dev: dev float [D] (read for standard columns only).  A workgroup owns 32 columns and a
 * chunk of rows and searches its columns' knots in LDS ([Q][32]: conflict-free); one read and one write of the matrix, no atomics,
 * no dependence on the launch geometry.  OSD_EINVAL, before any launch: a NULL pointer, Q outside [2, OSD_XF_MAX_Q], D < 1, rows < 0,
 * ld < D, a kind other than the three (the kinds are read back first).  rows == 0 is OSD_OK without a launch.  The kernel is left
 * running on `stream`. */
#define OSD_XF_IDENTITY        0
#define OSD_XF_STANDARD        1
#define OSD_XF_QUANTILE_NORMAL 2
#define OSD_XF_MAX_Q           1024
int osd_xf_apply(void *stream, int device, const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int64_t rows, int D,
                 const int32_t *kind_dev, const float *knots_dev, int Q, const float *levels_dev,
                 const float *center_dev, const float *scale_dev, int inverse);

/* ---- biological constraint losses (north_star) ------------------------------
 * The reference declares them at models/cvae.py:262-302 as stubs that return 0.0 (and the diffusion
 * model has none), so nothing is added unless osd_set_constraints() configures them:
 *   pathway coherence    L_pc = mean_P (1 - c_P), c_P = mean off-diagonal Pearson correlation over the
 *                        batch rows of the member columns of pathway P (utils/validation.py:144-173);
 *                        pathways with fewer than 2 members are skipped
 *   mutation-expression  L_me = mean_{i in A, j in B} (corr_recon(i,j) - corr_true(i,j))^2
 *                        ("MSE on correlation matrices", models/cvae.py:296-297), |A|, |B| <= 64
 * Columns are indices into the D-wide feature vector; constant columns count as correlation 0. */
typedef struct osd_constraints {
  const int32_t *pathway_offsets;   /* host int32[n_pathways + 1], CSR over pathway_members */
  const int32_t *pathway_members;   /* host int32[offsets[n_pathways]] */
  int32_t n_pathways;               /* 0 disables the pathway term */
  double pathway_weight;            /* config.yaml:58 pathway_coherence_weight */
  const int32_t *cols_a;            /* host int32[n_a], e.g. mutation columns */
  const int32_t *cols_b;            /* host int32[n_b], e.g. pathway-score or expression columns */
  int32_t n_a, n_b;                 /* 0 disables the mutation-expression term */
  double mutexpr_weight;            /* config.yaml:59 mutation_expression_weight */
} osd_constraints;
/* Configures (c == NULL: clears) the terms osd_train_loss_fwd_bwd adds to the eps-MSE, evaluated on
 * x0_hat = (x_t - sqrt(1-ac_t) eps_hat) / sqrt(ac_t) (models/diffusion.py:405; P x_t + Q out under osd_set_prediction) against x0 of the batch:
 * loss = mse + pathway_weight * L_pc + mutexpr_weight * L_me, gradients flow into eps_hat. */
int osd_set_constraints(osd_handle *h, const osd_constraints *c);
/* (mse, L_pc, L_me) of the last osd_train_loss_fwd_bwd call; synchronises the handle's stream.  With osd_set_loss, parts[0] is the
 * configured eps-loss. */
int osd_get_loss_parts(osd_handle *h, float *parts_host3);

/* ---- the eps-loss of osd_train_loss_fwd_bwd ------------------------------------------------------------------------
 * With d = eps_hat - eps, row r at timestep t_r, n rows and D features:
 *   loss = 1/(n D) * sum_r w[t_r] * sum_f rho(d_rf),      dL/d eps_hat_rf = loss_scale/(n D) * w[t_r] * rho'(d_rf)
 *   OSD_LOSS_L2     rho = d^2                                                rho' = 2 d              (F.mse_loss; the default)
 *   OSD_LOSS_L1     rho = |d|                                                rho' = sign(d), 0 at 0  (F.l1_loss)
 *   OSD_LOSS_HUBER  rho = d^2 / 2 if |d| <= delta, else delta (|d| - delta/2)  rho' = clamp(d, -delta, delta)  (F.huber_loss)
 * t_weights_host: T non-negative finite per-timestep weights (host memory, copied), gathered by each row's timestep index (the
 * caller's t_index or the one drawn inside the call), or NULL: every row weighs 1.  The mean is over n D; it is NOT renormalised by
 * the sum of the weights.  huber_delta must be positive and finite for every kind (1.0 is the conventional default).
 * Persistent on the handle until the next osd_set_loss; synchronises the handle's stream.  OSD_LOSS_L2 with NULL weights is the state
 * of a new handle and runs exactly the kernels of a handle that never called this; anything else runs the loss epilogue (EpiLoss,
 * csrc/epilogues.h) in the same launch and sets OSD_TP_LOSS_EPI.  The constraint losses are added on top as before.
 * OSD_EINVAL: unknown kind, huber_delta <= 0 or not finite, a negative or non-finite weight. */
#define OSD_LOSS_L2    0
#define OSD_LOSS_L1    1
#define OSD_LOSS_HUBER 2
int osd_set_loss(osd_handle *h, int kind, double huber_delta, const float *t_weights_host);

/* ---- training on incomplete rows -----------------------------------------------------------------
 * enable != 0: a NaN element of x0 means "not observed" (MissDiff, Ouyang et al. 2023).  With m = !isnan(x0), x~0 = m ? x0 : 0:
 *   x_t    = a_t x~0 + b_t eps                                 (two rounded products, one add: osd_q_sample on x~0)
 *   target = eps | a_t eps - b_t x~0 | x~0                     (osd_set_prediction), kept in the workspace with NaN where m is false
 *   loss   = 1/(n D) * sum_r w[t_r] * sum_f m_rf rho(out_rf - target_rf)
 *   dL/d out_rf = m_rf * loss_scale/(n D) * w[t_r] * rho'(.)   (exactly 0 where m is false)
 * for every kind and weight table of osd_set_loss.  The NaN in the target buffer is the mask: no mask tensor exists.  The mean stays
 * over n D -- NOT the number of observed elements -- so every observed element of a dataset weighs the same whichever batch it lands
 * in, an all-missing batch gives loss 0 and zero gradients, and loss_scale keeps its meaning under data parallel.  A resident batch
 * source (osd_train_batch_source) is mixed first, NaN propagating: a mixed element is observed iff both parents are.  Inf is not a
 * marker and conditions must be finite.  With an all-finite batch x_t and the target have the bits of the unmasked call.
 * Such a call runs the masked q_sample kernels and the masked loss epilogue (EpiLossT<true>, csrc/epilogues.h; the default l2 objective
 * too) on the fp32 launcher -- also under "precision" 1, whose weight gradients are unaffected --, reads the target from the workspace
 * even when the caller injected eps, and sets OSD_TP_MASKED | OSD_TP_LOSS_EPI.  osd_q_sample_target follows the setting.
 * OSD_EUNSUPPORTED, before any launch and before any gradient buffer is touched: osd_train_loss_fwd_bwd with constraint losses
 * configured (batch statistics over x0^ and x0) or with gradients under osd_set_dp_clip; osd_row_sq_error and osd_bound_sweep.
 * Persistent on the handle like osd_set_loss; host state only, no synchronisation.  0, the state of a new handle, restores exactly the
 * launches of a handle that never called this.  OSD_EINVAL: a null handle. */
int osd_set_loss_mask(osd_handle *h, int enable);

/* ---- a logistic link on the leading output columns -------------------------------------------------
 * Columns [0, n_logistic) of the network's output are logits of a Bernoulli mean E[x0 | x_t] -- the 0/1 mutation block of the feature
 * vector -- instead of an unbounded x0^.  0, the state of a new handle, turns the link off and restores exactly the launches of a
 * handle that never called this.  Needs the prediction type OSD_PRED_SAMPLE.  With o the output, y the target, M = n_logistic:
 *   training   f <  M:  rho = max(o, 0) - o y + log1p(exp(-|o|))       d rho / d o = sigma(o) - y        (cross-entropy on the logit)
 *              f >= M:  rho(o - y) of osd_set_loss, as without a link
 *              loss = 1/(n D) * sum_r w[t_r] * sum_f rho_rf;  dL/d out its exact derivative times loss_scale.  The weights, the NaN
 *              mask of osd_set_loss_mask, a resident batch source and its mixup (y inside [0, 1]) keep their meaning.  One launch, as
 *              before (EpiLossT<true, true>, csrc/epilogues.h), on the fp32 launcher whatever "precision" says; the call sets
 *              OSD_TP_LINK | OSD_TP_LOSS_EPI.
 *   sampling   osd_sample_chain_clipped and osd_sample_chain_multistep: x0 = sigma(P x + Q o) on the columns f < M, in front of the
 *              clamp; the update, the history store and the known overwrite follow unchanged, so every returned value of those
 *              columns lies in [0, 1] whatever the bounds.  Guidance combines raw outputs: it acts on the logit there.
 *   osd_convert_prediction: x0^ = sigma(o) on those columns; eps^ and v^ are derived from that x0^.
 * OSD_EUNSUPPORTED, before any launch: every entry point that folds x0^ away or reads the output as x0^ -- osd_p_sample_step,
 * osd_sample_chain, _steps, _guided, _known (the clipped entry points take their arguments; infinite bounds leave a column free);
 * osd_train_loss_fwd_bwd with constraint losses configured or with gradients under osd_set_dp_clip; osd_row_sq_error and
 * osd_bound_sweep (no likelihood bound for a Bernoulli block: refused, not approximated).
 * Host state only, read when the next call is issued, like osd_set_loss_mask.  OSD_EINVAL: a null handle, n_logistic outside [0, D],
 * or n_logistic > 0 while the handle's type is not OSD_PRED_SAMPLE; as either can be set second, the calls above return OSD_EINVAL
 * for that combination as well. */
int osd_set_output_link(osd_handle *h, int n_logistic);

/* ---- the per-patient likelihood bound ----------------------------------------------------------
 * se[r] = sum_d (out[r][d] - target[r][d])^2: an eval-mode forward of q_sample(x0, t_r) and the per-row squared error of the network's
 * raw output against the training target of the current prediction type (eps, a eps - b x0 or x0), in the launch of output_proj
 * (EpiRowSq, csrc/epilogues.h).  No float atomics: two calls on the same inputs return equal bits.  Both entry points are the
 * loss-only training call with that epilogue: no dropout, no gradients; they ignore osd_set_loss and osd_set_constraints and leave
 * them as they were, and they consume no armed osd_train_batch_source / osd_train_condition_dropout -- OSD_ESTATE while one is armed
 * (it stays armed).  fp32 kernels only: OSD_EUNSUPPORTED under "precision" 1.  Asynchronous on the handle's stream.
 * Generated noise (noise_in NULL): the normals of element quad c >> 2 of patient i at timestep t are the Philox block
 * (seed, row_offset + i, c >> 2, t, q_sample's tag) -- a draw depends on (seed, global patient id, timestep) alone, not on the
 * chunking, on S, or on how a cohort is split over calls.
 * OSD_EINVAL: a null tensor, n < 1, S < 1, a timestep outside [0, T), row_offset + n outside the 32-bit id space.
 *   t_index   dev int32 [n], clamped into [0, T)
 *   noise_in  dev [n][D], or NULL
 *   se_out    dev [n] */
int osd_row_sq_error(osd_handle *h, const float *x0, const float *cond, int64_t n, const int32_t *t_index,
                     const float *noise_in, uint64_t seed, int64_t row_offset, float *se_out);
/* The same for every (timestep, patient) pair: se_out dev [S][n], noise_in dev [S][n][D] or NULL, timesteps_host S host values.  The
 * rows of a launch are pairs in that order, x0 and cond are gathered from the patient (never replicated S times), and at most
 * "bound_rows" rows go into one launch group, so the workspace is bounded for any n x S; a group may end inside a timestep. */
int osd_bound_sweep(osd_handle *h, const float *x0, const float *cond, int64_t n, const int32_t *timesteps_host, int S,
                    const float *noise_in, uint64_t seed, int64_t row_offset, float *se_out);

/* ---- the edit-friendly noise map of a patient -----------------------------------------------------
 * Turns n patients into a start state and the draws with which osd_sample_chain_steps (and the guided, known and clipped chains), run on
 * the SAME plan and condition, returns them: the DDPM noise space of Huberman-Spiegelglas et al. 2024.  timesteps_host [n_steps] and
 * step_coef_host [n_steps][4] = (A_s, B_s, C_s, 0) are exactly that plan; nothing is folded here, so the map inverts the very rows the
 * chain runs, for every prediction type (the plan's (A, B) carry it).  With a[t], b[t] the buffers of osd_set_schedule and eps_s an
 * independent normal per (patient, level):
 *   y_s   = a[tau_s] * x0 + b[tau_s] * eps_s                       s = 0 .. n_steps-1
 *   out_s = denoiser(y_s, tau_s, cond)                             eval mode, fp32 kernels
 *   z_s   = (y_{s-1} - (A_s * y_s + B_s * out_s)) / C_s            s = 1 .. n_steps-1
 *   x_start_out = y_{n_steps-1};   noises_out[n_steps-1-s] = z_s   (the chain's draw order)
 * z_s is formed as fmaf(-B, out, fmaf(-A, y_s, y_{s-1})) * (1 / C): the chain's step fmaf(A, y, fmaf(B, out, C z)) taken back outermost
 * operation first, so the chain returns y_{s-1} to rounding.  Level 0 draws nothing (C_0 = 0 stays a requirement) and does not run: the
 * chain's last step returns A_0 y_0 + B_0 out_0, the model's x0^ at tau_0.
 * eps_s is noise_in [n_steps][n][D], or for NULL the Philox block (seed, row_offset + i, c >> 2, tau_s, q_sample's tag) of
 * osd_bound_sweep: a draw depends on (seed, global patient id, timestep) alone.
 * The call is the loss-only training call of osd_bound_sweep with another q_sample pass and another output_proj epilogue (EpiNoiseMap,
 * csrc/epilogues.h): rows are (level, patient) pairs of the levels 1 .. n_steps-1 in that order, x0 and cond are gathered, at most
 * "bound_rows" rows go into one launch group and a group may end inside a level; y_{s-1} is recomputed from x0 in the row that needs it,
 * so groups are independent.  z is written straight into noises_out; neither the network output nor a posterior mean reaches memory.  No
 * atomics: two calls return equal bits, and a row's result does not depend on its group, chunk or shard.  Asynchronous on the handle's
 * stream.  Ignores osd_set_loss, osd_set_constraints and osd_set_loss_mask and leaves them as they were.
 * OSD_EINVAL, all checked on the host before any device call: a null tensor, n < 1, n_steps outside [1, T], timesteps not strictly
 * increasing or outside [0, T), a non-finite coefficient, C_0 != 0, C_s <= 0 for some s >= 1 (the map needs eta > 0), row_offset + n
 * outside the 32-bit id space.  OSD_ESTATE: osd_train_batch_source / osd_train_condition_dropout is armed (it stays armed).
 * OSD_EUNSUPPORTED: "precision" 1, or an output link (a linked model's step is not the plain affine row: refused, not approximated).
 *   x0, cond      dev [n][D], [n][condition_dim]
 *   noise_in      dev [n_steps][n][D], or NULL
 *   x_start_out   dev [n][D]
 *   noises_out    dev [n_steps-1][n][D] (may be NULL when n_steps == 1) */
int osd_noise_map(osd_handle *h, const float *x0, const float *cond, int64_t n, const int32_t *timesteps_host,
                  const float *step_coef_host, int32_t n_steps, const float *noise_in, uint64_t seed, int64_t row_offset,
                  float *x_start_out, float *noises_out);
/* Stand-alone ops (stream/device based, synchronous): loss_out (dev float[1]) += weight * L and, when
 * dx != NULL, dx (dev [rows][ld]) += weight * dL/dx.  x, x_recon, x_true: dev [rows][ld], cols <= ld. */
int osd_loss_pathway_coherence(void *stream, int device, const float *x, int64_t rows, int ld, int cols,
                               const int32_t *offsets_host, const int32_t *members_host, int n_pathways,
                               double weight, float *loss_out, float *dx);
int osd_loss_mutation_expression(void *stream, int device, const float *x_recon, const float *x_true,
                                 int64_t rows, int ld, int cols, const int32_t *cols_a_host, int n_a,
                                 const int32_t *cols_b_host, int n_b, double weight, float *loss_out,
                                 float *dx);

/* ---- layer ops behind the cVAE mirror (models/cvae.py) -----------------------
 * Stream/device based, asynchronous (nothing synchronises), every tensor a device pointer. */
/* torch.cat([x1, x2], -1) -> nn.Linear (models/cvae.py:54-55, 97-98): y[n][N] = [x1|x2] w[N][K1+K2]^T + b.
 * K2 == 0: plain Linear (x2 ignored). */
int osd_nn_linear(void *stream, int device, const float *x1, int K1, const float *x2, int K2,
                  const float *w, const float *b, int64_t n, int N, float *y);
/* Its backward: dw[N][K1+K2] = gy^T [x1|x2] (overwritten), db[N] = column sums of gy (NULL: skipped),
 * dx1[n][K1] = gy w[:, :K1] (NULL: skipped; the x2 panel -- the conditions -- gets no gradient). */
int osd_nn_linear_bwd(void *stream, int device, const float *x1, int K1, const float *x2, int K2,
                      const float *w, const float *gy, int64_t n, int N, float *dx1, float *dw, float *db);
/* nn.BatchNorm1d -> nn.ReLU -> nn.Dropout (models/cvae.py:29-32, 79-82) on z[n][C].
 *   training != 0: batch statistics (biased variance), running_mean/var updated with `momentum`
 *                  (unbiased variance), dropout from `mask` (dev float 0/1 keep-mask [n][C]) or, when
 *                  mask == NULL, Philox(seed, tag); n >= 2 required as in torch
 *   training == 0: running statistics, no dropout
 *   use_bn == 0:   ReLU -> Dropout only (the survival head, models/cvae.py:251-252)
 * save_mean / save_invstd (dev float[C]) receive the statistics the backward needs. */
int osd_nn_bn_relu_dropout(void *stream, int device, const float *z, int64_t n, int C, const float *gamma,
                           const float *beta, float *running_mean, float *running_var, double momentum,
                           double eps, int training, int use_bn, double p_drop, const float *mask,
                           uint64_t seed, uint32_t tag, float *y, float *save_mean, float *save_invstd);
int osd_nn_bn_relu_dropout_bwd(void *stream, int device, const float *gy, const float *z, int64_t n, int C,
                               const float *gamma, const float *beta, const float *save_mean,
                               const float *save_invstd, int training, int use_bn, double p_drop,
                               const float *mask, uint64_t seed, uint32_t tag, float *dz, float *dgamma,
                               float *dbeta);
/* reparameterize (models/cvae.py:152-156): z = mu + eps * exp(0.5 * logvar); eps_in NULL -> Philox(seed)
 * normals, written to eps_out when it is not NULL. */
int osd_nn_reparameterize(void *stream, int device, const float *mu, const float *logvar, const float *eps_in,
                          uint64_t seed, int64_t n, int Lz, float *z, float *eps_out);
/* Backward of reparameterize: d_logvar = 0.5 * gz * eps * exp(0.5 * logvar)   (d_mu is gz itself).  eps is the noise the
 * forward used (eps_in, or what it wrote to eps_out); it is never recovered as z - mu, which cancels when |mu| >> std. */
int osd_nn_reparameterize_bwd(void *stream, int device, const float *gz, const float *eps, const float *logvar,
                              int64_t count, float *d_logvar);
/* VAE loss (models/cvae.py:178-181): parts3 (dev float[3]) = (recon + kl, recon, kl) with
 * recon = sum (x_recon - x)^2 / n, kl = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) / n, and their
 * gradients d_recon[n][D], d_mu[n][Lz], d_logvar[n][Lz] (each may be NULL). */
int osd_nn_vae_loss(void *stream, int device, const float *x_recon, const float *x, const float *mu,
                    const float *logvar, int64_t n, int D, int Lz, float *parts3, float *d_recon,
                    float *d_mu, float *d_logvar);
/* One tensor of MixupAugmentation.__call__ (utils/train.py:108-120) without a model handle:
 * out[rows][cols] = lam * v + (1 - lam) * v[perm]. */
int osd_nn_mixup(void *stream, int device, const float *v, const int64_t *perm, double lam, int64_t rows,
                 int cols, float *out);
/* The three tensors of one MixupAugmentation call (data [rows][data_cols], conditions [rows][cond_cols], survival [rows]) in
 * ONE launch; a NULL output skips that tensor. */
int osd_nn_mixup3(void *stream, int device, const float *data, const float *cond, const float *surv,
                  const int64_t *perm, double lam, int64_t rows, int data_cols, int cond_cols,
                  float *data_out, float *cond_out, float *surv_out);
/* F.mse_loss(a, b) over `count` elements (models/cvae.py:323): loss_out dev float[1], da (may be NULL). */
int osd_nn_mse(void *stream, int device, const float *a, const float *b, int64_t count, float *loss_out,
               float *da);

/* ---- building blocks, exported for the parity tests ------------------------ */
/* y[n][N] = act(x[n][K] @ w[N][K]^T + b), act = identity (silu=0) or SiLU. */
int osd_op_linear(osd_handle *h, const float *x, const float *w, const float *b, int64_t n, int K,
                  int N, int silu, float *y);
/* Linear -> GroupNorm(8) -> SiLU, one half of _make_block (models/diffusion.py:200-203).
 * x2/K2: optional second K panel (concat-free decoder input, :250). */
int osd_op_linear_gn_silu(osd_handle *h, const float *x, int K1, const float *x2, int K2,
                          const float *w, const float *b, const float *gamma, const float *beta,
                          int64_t n, int N, float *y);
/* C[p][f] (+)= sum_k A(f,k) B(p,k), C row-major [P][F] with leading dimension ldc;
 * a_kc/b_kc: operand stored [row][k] (1) or [k][row] (0).  Forward Linear is (1,1),
 * dgrad (0,1), wgrad (0,0). */
int osd_op_gemm(osd_handle *h, const float *A, int lda, int a_kc, const float *B, int ldb, int b_kc,
                int F, int P, int K, float *C, int ldc, int accumulate);
/* out[rows][cols] standard normals from the library's Philox stream, addressed by
 * (seed, row_offset + row, col/4, step, kind): kind 0 = the z of p_sample at t == step
 * (step == T is x_T), 1 = the eps of q_sample (step 0), >= 2 = user streams. */
int osd_op_randn(osd_handle *h, float *out, int64_t rows, int cols, uint64_t seed,
                 int64_t row_offset, uint32_t step, uint32_t kind);

#ifdef __cplusplus
}
#endif
#endif /* OSDIFF_H */
