// handle.h -- host-side state behind osd_handle.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/osdiff.h"
#include "batch_src.h"

namespace osd {

void set_error(const char* fmt, ...);

#define OSD_HIP(call)                                                                    \
  do {                                                                                   \
    hipError_t e__ = (call);                                                             \
    if (e__ != hipSuccess) {                                                             \
      ::osd::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      (void)hipGetLastError(); /* reported: do not let it resurface in a later launch check */            \
      return OSD_EHIP;                                                                   \
    }                                                                                    \
  } while (0)

#define OSD_TRY(call)               \
  do {                              \
    int r__ = (call);               \
    if (r__ != OSD_OK) return r__;  \
  } while (0)

inline int64_t up64(int64_t v) { return (v + 63) / 64 * 64; }      // buffers are carved in whole 64-float (256-byte) granules
// hipMalloc that reports: OSD_ENOMEM with the byte count in osd_last_error(), the sticky HIP error cleared
int device_alloc(void** p, size_t bytes);

}  // namespace osd

#include "devmem.h"
#include "constraints.h"

namespace osd {

// One Linear of the denoiser trunk (with or without GroupNorm+SiLU behind it).
struct LayerDesc {
  int K1, K2;          // input panel widths (K2 > 0: concat-free decoder input)
  int N;               // output width
  int w, b;            // parameter indices
  int gamma, beta;     // -1 when no GroupNorm
  int gw;              // channels per group (N/8) when GroupNorm
  int block;           // block index (execution order) or -1
  int half;            // 0 first Linear of the block (dropout behind it), 1 second
};

// Parameter indices in named_parameters() order.
struct ParamMap {
  int ce0_w, ce0_b, ce2_w, ce2_b;
  int in_w, in_b, cp_w, cp_b, tp_w, tp_b;
  int out_w, out_b;
  int n_params;
  std::vector<int64_t> numel;
};

struct Arch {
  int D, H0, cond_dim, time_dim, cond_width, T;
  int n_blocks, n_enc;
  std::vector<int> hidden;
  std::vector<LayerDesc> layers;   // 2 per block, execution order
  std::vector<int> block_out;      // output width of block i
  ParamMap pm;
  int64_t act_floats_per_row;      // forward workspace per row
  // the encoder block whose output decoder block b concatenates (LIFO: decoder j pops encoder n_enc - 1 - j)
  int skip_of(int b) const { return n_enc - 1 - (b - n_enc - 1); }
};

int build_arch(const osd_config& cfg, Arch* a);

// What one reverse chain runs: n_steps steps t = n_steps - 1 .. 0, step t reading row t of temb [n_steps][H0]
// (time_proj(TimeEmbedding(tau / T)) of the step's timestep tau) and of coef [n_steps][4] = (A, B, C, 0), x' = A x + B eps + C z.
// Philox draws of step t use step counter t, injected draws sit at noises[n_steps - 1 - t].  The DDPM chain of osd_sample_chain
// is {T, d_temb, d_coef}; osd_sample_chain_steps gathers a strided plan into the handle's plan_temb / plan_tab.
struct StepPlan {
  int n_steps;
  const float* temb;
  const float* coef;
};

// Classifier-free guidance of a chain / an evaluation (osd_sample_chain_guided): eps = eps(c0) + w * (eps(c) - eps(c0)).
struct Guide {
  const float* null_cond;      // dev [cond_dim]; null = unguided
  float w;
};

// Known-feature conditioning of a chain (osd_sample_chain_known): observed elements are overwritten after every step (EpiPosterior<POST_PLAIN, true>).
struct Known {
  const float* known;          // dev [n][ld], NaN = free; null = nothing known
  int64_t ld;
  const float* level;          // dev [S][2]
};

// Clipping of the predicted x0 to per-feature bounds inside the posterior launch (osd_sample_chain_clipped, EpiPosterior<POST_CLIP>).
struct Clip {
  const float* bounds;         // dev [2][ld]: the lo row, then the hi row; null = no clipping
  int ld;
  const float* x0_coef;        // dev [S][4] = (P, Q, E, F)
  int n_link;                  // columns [0, n_link) of the output are logits (osd_set_output_link): sigma before the clamp; 0 = none
};

// The DPM-Solver++(2M) multistep update (osd_sample_chain_multistep, EpiPosterior<POST_HIST>): the chain keeps the previous step's clipped x0.
// Always with a Clip, whose x0_coef rows are then (P, Q, G, F) and whose bounds may be all-infinite.
struct Multistep {
  const float* hist_coef;      // dev [S] = H; null = single-step chains
};

// One reverse-chain request, as every sampler engine receives it (api.hip: sample_request fills it from an entry point's arguments).
struct ChainJob {
  StepPlan plan;
  const float* cond; int64_t n; const float* x_T; const float* noises; uint64_t seed; int64_t row_offset;
  float* x_out; float* mut_mask_out; int flags;
  Guide guide;
  Known known;
  Clip clip;
  Multistep multistep;
  int D, cond_dim, mutation_dim;   // row widths of x_T / noises / x_out, of cond and of mut_mask_out
  int64_t n_total;                 // rows of the whole request: injected draws of consecutive steps lie n_total * D floats apart
  // rows [r0, r0 + m) of the request as a job of their own
  ChainJob chunk(int64_t r0, int64_t m) const {
    ChainJob c = *this;
    c.n = m; c.row_offset = row_offset + r0;
    c.cond = cond + r0 * cond_dim;
    c.x_out = x_out + r0 * D;
    if (x_T) c.x_T = x_T + r0 * D;
    if (noises) c.noises = noises + r0 * D;
    if (mut_mask_out) c.mut_mask_out = mut_mask_out + r0 * mutation_dim;
    if (known.known) c.known.known = known.known + r0 * known.ld;
    return c;
  }
};

// Forward activations of one row chunk (all device pointers into one arena).
struct FwdWs {
  float* ce1;     // [n][64]   SiLU(Linear(cond))
  float* ce2;     // [n][64]   condition embedding
  float* cproj;   // [n][H0]
  float* h0;      // [n][H0]
  std::vector<float*> mid;   // per block: first-half output (post dropout)  [n][C]
  std::vector<float*> out;   // per block: block output                      [n][C]
  // training extras (null in inference)
  std::vector<float*> z1, z2;        // pre-norm activations of both halves
  std::vector<float*> st1, st2;      // (mean, rstd) [n][8][2]
};

struct Slot {
  Stream stream;                     // h->main has none: the single-stream entry points run on the caller's
  Event done;
  DevBuf<float> arena;
  DevBuf<int> t_dev;
  Graph graph;                       // graph of the last captured reverse step (kept alive
  GraphExec exec;                    // until its replays have drained)
};

}  // namespace osd

struct osd_handle {
  osd_config cfg;
  osd::Arch arch;
  hipStream_t stream = nullptr;
  std::vector<const float*> params;
  bool have_schedule = false, have_weights = false;
  osd::DevBuf<float> w_in_packed;    // input_proj.weight zero-padded to [H0][roundup(D,32)] for the LDS-DMA kernel
  int w_in_ld = 0;
  bool w_packed_stale = false;      // a training step skipped the repack of w_in_packed / w_out_packed: refreshed lazily (api.hip: ensure_packed)
  // D % 4 != 0 (e.g. the reference's real dims 62 + 5054 + 26 = 5142): the reverse chain keeps its state in an internal buffer
  // whose rows are padded to Dp = roundup(D, 4) floats, so that every operand is 16-byte aligned and the LDS-DMA / FAST tile code
  // and the chain kernel apply; the pad columns carry finite values that only ever meet zero weights
  int Dp = 0;
  int cond_bwd_fused = 1;            // osd_set_option("cond_bwd_fused", 0|1): the conditioning branch's backward below h0 as one launch (k_cond_bwd, k_train.hip)
  bool sq_wpk_t_fresh = false;       // the backward squads' transposed weight copies were packed by this step's forward launch (chain_squad.hip)
  bool splitk_suspended = false;     // a chain-kernel fallback re-run in progress: no split-K (bit-identical to the chain kernel)
  int input_splitk = 0;              // osd_set_option("input_splitk"): 0 off (default: a row's result does not depend on how rows are chunked / sharded),
                                     // -1 auto (chunks with < 128 input_proj tiles), n = slices
  osd::DevBuf<float> w_out_packed;   // [Dp][H_last]: output_proj.weight + zero rows for the pad columns (allocated iff D % 4)
  osd::DevBuf<float> b_out_packed;   // [Dp]
  osd::DevBuf<float> chain_xpad;     // padded chain state of the chain kernel [n][Dp]
  osd::DevBuf<float> d_sqrt_ac, d_sqrt_1m, d_coef, d_time_emb, d_temb;
  // the step plan of osd_sample_chain_steps (StepPlan): gathered temb rows [T][H0], and the uploaded table of an S-step plan:
  // coefficients [S][4], then timesteps [S] (as int32)
  osd::DevBuf<float> plan_temb;
  osd::Staged<float> plan_tab;
  int64_t chunk_rows = 65536;
  int n_streams = 2;
  std::vector<osd::Slot> slots;
  osd::Slot main;            // workspace used by the single-stream entry points
  osd::Event fork_ev;
  // training workspace
  osd::DevBuf<float> train_arena;
  osd::DevBuf<float> loss_dev;
  osd::DevBuf<int> t_san;            // clamped copy of a caller-supplied t_index (sanitize_t)
  osd::DevBuf<double> normsq_dev;    // 256 per-workgroup partials of the gradient norm (osd_clip_adamw_step)
  // weight-gradient side stream of the backward pass and its fork/join events
  osd::Stream wgrad_stream;
  std::vector<osd::Event> ev_pool;
  int train_streams = 2;             // osd_set_option("train_streams", 1|2): 2 = weight-gradient leaves of the backward pass on a side stream
  osd::BatchSrc batch_src{}; bool have_batch_src = false;      // osd_train_batch_source: one-shot source of the next training call's rows
  // classifier-free guidance: the null condition -- slot 0 of the current guided sampling / forward call, slot 1 of the next training
  // call's condition dropout (each cond_dim floats, 64-float stride) (api.hip: upload_null_cond)
  osd::Staged<float> null_cond;
  bool null_valid[2] = {false, false};      // the device slot holds the staging's vector: a call with the same bits uploads nothing
  // known-feature conditioning (osd_sample_chain_known): the schedule's two level buffers as osd_set_schedule received them, and the
  // current call's level table [S][2]
  std::vector<float> sched_sqrt_ac, sched_sqrt_1m;
  osd::Staged<float> known_level;
  // x0 clipping (osd_sample_chain_clipped): the DDPM chain's (P, Q, E, F) rows [T][4] folded by osd_set_schedule, and the current call's
  // tables -- coefficients [T][4], then bounds [2][Dp] (pad columns (-inf, +inf))
  std::vector<float> sched_x0_coef;
  osd::Staged<float> clip_tab;
  // the multistep solver (osd_sample_chain_multistep): the current call's history coefficients [T]
  osd::Staged<float> hist_coef;
  bool have_cond_drop = false; float cond_drop_p = 0.f; const float* cond_drop_keep = nullptr;   // osd_train_condition_dropout: one-shot
  int64_t saved_rows = -1;           // rows of the last osd_denoiser_forward_train whose activations are still in the arena
  // constraint losses (osd_set_constraints); parts_dev = (mse, L_pc, L_me) of the last training call
  osd::ConsPlan cons;
  double w_pathway = 0.0, w_mutexpr = 0.0;
  osd::DevBuf<float> parts_dev;
  // the eps-loss of the training step (osd_set_loss): persistent.  loss_kind OSD_LOSS_*, loss_tw = per-timestep weights [T] on the device while
  // a table is set (loss_tw_set), else every row weighs 1.  OSD_LOSS_L2 without a table is the default and runs EpiMse
  // what the network predicts (osd_set_prediction): persistent.  pred_type OSD_PRED_*; sched_post_coef = the six per-step scalars as
  // osd_set_schedule received them, from which fold_schedule (api.hip) refolds d_coef / sched_x0_coef / d_pq for the type.  d_pq: dev
  // (P, Q) [T][2] of x0^ = P x_t + Q out (the constraint losses), then the (U, V) [T][2] of osd_convert_prediction for conv_kind (-1: none)
  int pred_type = 0; std::vector<float> sched_post_coef;
  osd::DevBuf<float> d_pq; int conv_kind = -1;
  int loss_kind = 0; float loss_delta = 1.0f;
  osd::DevBuf<float> loss_tw; bool loss_tw_set = false;
  // training on incomplete rows (osd_set_loss_mask): persistent.  NaN in x0 = not observed; the q_sample kernels zero-fill it and mark the
  // target with NaN, the loss runs EpiLossT<true> on the fp32 launcher.  false: today's launches
  bool loss_mask = false;
  // logistic link on the leading output columns (osd_set_output_link): persistent.  Columns [0, n_link) of the output are logits of a
  // Bernoulli mean: cross-entropy in the training loss (EpiLossT<true, true>), sigma in front of the clamp of the x0-unfolded posterior
  // launches and in osd_convert_prediction.  0: today's launches.  Needs OSD_PRED_SAMPLE; either can be set second, so the calls check
  int n_link = 0;
  // differentially private training (osd_set_dp_clip; dp.h): persistent.  dp_clip = the per-row gradient bound C (0: off, today's launches);
  // dp_norms = dev [2][dp_norms.cap() / 2]: s_r, then the clip factors c_r, of the last clipped call's dp_rows rows (-1: none yet); dp_plan = the
  // cached item lists of the two launches (k_dp.hip)
  double dp_clip = 0.0;
  osd::DevBuf<float> dp_norms; int64_t dp_rows = -1;
  void* dp_plan = nullptr;
  bool dp_replay_ok = false;         // osd_dp_replay: the lists still describe the workspace (cleared by whatever carves it again: ensure_train_ws)
  // the likelihood bound (osd_row_sq_error / osd_bound_sweep) and the noise map: rows per launch group, and the call's timesteps on the device
  int64_t bound_rows = 32768;        // osd_set_option("bound_rows")
  osd::DevBuf<int> bound_ts;
  // the noise map (osd_noise_map): the call's step_coef rows on the device, next to its timesteps in bound_ts
  osd::DevBuf<float> map_coef;
  std::vector<void*> wg_plans;       // grouped weight-gradient launches (wgrad_group.hip): one cached work list per flush point
  // persistent reverse-chain kernel (chain.h / chain.hip)
  int sampler = 0;                   // osd_set_option("sampler"): 0 auto, 1 chain kernel whenever the architecture allows, 2 per-layer kernels
  int chain_grid = 0;                // 0 = min(row tiles, resident slots); > 0 caps the workgroup count (tests: force cross-workgroup hand-offs)
  int chain_steps_per_launch = 0;    // 0 = the whole chain in one launch
  int chain_stagger = 30000;         // shader cycles between the starts of the two workgroups of a CU (0 = off)
  osd::DevBuf<float> chain_ws;
  osd::DevBuf<float> chain_cond;
  osd::DevBuf<unsigned> chain_sync;
  // argument blocks of the chain kernels' launches (ChainArgs / PanelArgs / SquadArgs), one per launch of the current chain: device
  // copies the kernels read and host copies kept alive while their uploads may be pending (chain.hip: chain_args_ring)
  osd::DevBuf<char> chain_args_dev; std::vector<char> chain_args_host;
  bool chain_pending = false;        // a chain was launched whose status word has not been read yet
  unsigned long long chain_spin_budget = 500000000ull;   // osd_set_option("chain_spin_budget"): s_memrealtime ticks (100 MHz) a dependency wait may take (5 s)
  int64_t chain_wall_budget_ms = 0;  // osd_set_option("chain_wall_budget_ms"): host-side budget of a synchronous chain; 0 = 10 x the expected run time + 2 s
  double chain_expected_ms = 0.0;    // run-time estimate of the chain launched last (chain_run)
  int64_t chain_fallbacks = 0;       // chains that gave up and were re-run on the per-layer kernels (osd_get_option)
  osd::Stream abort_stream;             // carries the host's abort flag to a chain kernel that overran its wall-clock budget
  unsigned long long* chain_stamps = nullptr;   // diagnostic builds (csrc/diag): device buffer of 8 counters per workgroup, else null
  int last_engine = 0;               // engine of the most recent osd_sample_chain (0 per-layer, 1 chain kernel)
  // LDS-resident variant of the chain kernel (chain_panel.h / chain_panel.hip)
  int chain_variant = 0;             // osd_set_option("chain_variant"): 0 auto (chain.hip: chain_use_panel / squad_window), 1 workspace chain (chain.h),
                                     // 2 LDS-resident chain where the architecture fits (else 1), 3 squad chain (chain_squad.h) where model and batch fit (else auto's choice without it)
  int last_chain_variant = 0;        // variant the most recent chain-kernel run used (osd_get_option)
  osd::DevBuf<float> panel_wpk;      // fragment-ordered copies of the weights
  bool panel_wpk_valid = false;      // false after anything that may have changed the parameters: repacked by the next chain
  // small-batch variant (chain_squad.h / chain_squad.hip)
  osd::DevBuf<float> squad_wpk[2];   // fragment-ordered weights: [0] 32-patient panels, [1] 16-patient panels
  bool squad_wpk_valid[2] = {false, false};
  int last_squad_rp = 0;             // patients per panel of the squad chain that ran last (osd_get_option "last_squad_panel")
  int train_squad = 2;               // osd_set_option("train_squad"): the training forward trunk as one launch of squads (train_squad.h) from 2 048 rows on
  int squad_panel = 0;               // osd_set_option("squad_panel"): 0 auto (16-patient panels up to one 32-patient workgroup per CU), 16, 32
  // bf16x3 split precision (gemm_bf3.h / split.hip)
  int precision = 0;                 // osd_set_option("precision"): 0 fp32 MFMA (default; the reference's arithmetic), 1 bf16x3 split on the bf16 matrix pipe
                                     // (fp32 accuracy, eval-mode sampling / forward of 256 / 512 wide trunks; everything else stays fp32)
  int last_precision = 0;            // precision the most recent forward / p_sample / sample call computed in (osd_get_option)
  int last_train_path = 0;           // OSD_TP_* bits: what the most recent osd_train_loss_fwd_bwd / osd_denoiser_backward ran (osd_get_option)
  void* split_plan = nullptr;        // weight planes (split.hip)
  bool split_valid = false;          // false after anything that may have changed the parameters: repacked by the next split-precision call
  // osd_profile_step: when non-null, run_trunk records prof_events[prof_i++] after every launch
  std::vector<hipEvent_t>* prof_events = nullptr;
  int prof_i = 0;
  ~osd_handle();                     // api.hip: the members release themselves; the opaque plans go through their *_free
};
