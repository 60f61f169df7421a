// kernels.h -- host-callable wrappers around the device kernels (one .hip file each group).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/osdiff.h"
#include "gemm.h"
#include "epilogues.h"
#include "batch_src.h"

namespace osd {

// k_linear.hip ---------------------------------------------------------------------
// out[p][f] (+)= act( sum_k A(f,k) B(p,k) + bias[f] ); layouts: a_kc/b_kc as in gemm.h
hipError_t launch_linear(hipStream_t s, const GemmArgs& g, bool a_kc, bool b_kc, const float* bias,
                         float* out, int ldo, bool silu, bool accumulate);

hipError_t launch_wgrad_splitk(hipStream_t s, const GemmArgs& g, float* slabs, int ldo, long long slice_stride);

// k_fused.hip ----------------------------------------------------------------------
hipError_t launch_input(hipStream_t s, const GemmArgs& g, const EpiInput::Args& a, bool a_zero_padded);
// a classifier-free-guidance step's input_proj: g.P = m state rows, 2 m output rows (EpiInputGuided); launch_input's tile choice
hipError_t launch_input_guided(hipStream_t s, const GemmArgs& g, const EpiInputGuided::Args& a, bool a_zero_padded);
hipError_t launch_input_guided_splitk(hipStream_t s, const GemmArgs& g, const EpiInputGuided::Args& a, float* slabs, int slices);
hipError_t launch_input_splitk(hipStream_t s, const GemmArgs& g, const EpiInput::Args& a, float* slabs, int slices);
// output_proj + one step of the reverse chain (EpiPosterior<MODE, KNOWN>), one tile choice.  The argument type picks MODE: plain, around
// observed values, with the predicted x0 clipped to per-feature bounds (KNOWN = a.known != null), the DPM-Solver++(2M) multistep
// update on the clipped x0 (KNOWN = a.c.known != null); the Link argument types add the logistic link to the last two
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorArgs& a);
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorKnownArgs& a);
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorClipArgs& a);
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorHistArgs& a);
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorClipLinkArgs& a);
hipError_t launch_posterior(hipStream_t s, const GemmArgs& g, const PosteriorHistLinkArgs& a);
hipError_t launch_mse(hipStream_t s, const GemmArgs& g, const EpiMse::Args& a);
// k_b3t.hip: precision = 1 (hipErrorInvalidValue: outside the kernel's preconditions -- run the fp32 launch)
hipError_t launch_mse_b3t(hipStream_t s, const GemmArgs& g, const EpiMse::Args& a);
// output_proj + the loss of osd_set_loss (EpiLoss): launch_mse's / launch_mse_b3t's tile choices and return values
hipError_t launch_loss(hipStream_t s, const GemmArgs& g, const EpiLoss::Args& a);
hipError_t launch_loss_b3t(hipStream_t s, const GemmArgs& g, const EpiLoss::Args& a);
// ... with the unobserved elements of a NaN-marked target left out (EpiLossT<true>; osd_set_loss_mask).  fp32 only.
hipError_t launch_loss_masked(hipStream_t s, const GemmArgs& g, const EpiLossT<true>::Args& a);
// ... and cross-entropy on the logits in columns [0, a.n_link) (EpiLossT<true, true>; osd_set_output_link).  fp32 only.
hipError_t launch_loss_link(hipStream_t s, const GemmArgs& g, const EpiLossT<true, true>::Args& a);
// output_proj + per-row squared error (EpiRowSq), launch_mse's tile choice, then k_rowsq_reduce: se[P].  a.part: rowsq_slots(F) x a.ld
// floats.  poison: a device word added to every row (0, or the NaN of a squad launch that gave up), or null.  fp32 only.
constexpr int ROWSQ_WF = 64;      // feature extent of a wave in both tiles of the tile choice
inline int rowsq_slots(int F) { return (F + ROWSQ_WF - 1) / ROWSQ_WF; }
hipError_t launch_row_sq(hipStream_t s, const GemmArgs& g, const EpiRowSq::Args& a, const float* poison, float* se);
// output_proj + the noise map's solve (EpiNoiseMap), launch_mse's tile choice: row p's z lands at a.z + a.row[p].zoff.  fp32 only.
hipError_t launch_noise_map(hipStream_t s, const GemmArgs& g, const EpiNoiseMap::Args& a);

// k_gn.hip / k_gn_drop.hip ------------------------------------------------------------
// Arguments common to every GW; the wrappers copy them into EpiGnSilu<GW,DROP>::Args.
struct GnArgs {
  const float* bias; const float* gamma; const float* beta;
  float* out; int ldo;
  float* z_out; int ldz; float* stats;
  int drop_mode; const float* mask; int ldm; float keep_scale; float p_drop;
  uint64_t seed; uint32_t row_offset; uint32_t step; uint32_t tag; const int* step_dev;
};
bool gn_width_supported(int gw);
hipError_t launch_gn_silu(hipStream_t s, const GemmArgs& g, int gw, const GnArgs& a);        // drop_mode == 0
hipError_t launch_gn_silu_drop(hipStream_t s, const GemmArgs& g, int gw, const GnArgs& a);   // drop_mode 1/2
// k_fused.hip: small batches -- K slices over workgroups + a reduce / GroupNorm / SiLU kernel (another fp32 summation order: opt-in)
hipError_t launch_gn_silu_splitk(hipStream_t s, const GemmArgs& g, const GnArgs& a, float* slabs, int slices);

// k_elem.hip -----------------------------------------------------------------------
hipError_t launch_set_int(hipStream_t s, int* p, int v);
hipError_t launch_add_int(hipStream_t s, int* p, int d);
hipError_t launch_gather_rows(hipStream_t s, const float* src, int cols, const int* idx, int rows, float* dst);   // dst[r] = src[idx[r]]
hipError_t launch_fill_randn(hipStream_t s, float* out, int ld, int64_t rows, int cols, uint64_t seed,
                             uint32_t row_offset, uint32_t step, uint32_t tag);
hipError_t launch_copy2d(hipStream_t s, const float* src, int lds, float* dst, int ldd, int64_t rows, int cols);
hipError_t launch_q_sample(hipStream_t s, const float* x0, const int* t, const float* sqrt_ac, const float* sqrt_1m,
                           const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset,
                           float* x_t, float* noise_out, int* t_out = nullptr, int T = 0, int ldxt = 0, const ZeroList* zl = nullptr,
                           int kind = OSD_PRED_EPSILON,       // kind != epsilon: noise_out receives the training target (k_elem.hip: q_target)
                           bool masked = false);              // NaN in x0 = not observed: zero-filled for x_t, NaN-marked in the target (any kind)
hipError_t launch_q_sample_src(hipStream_t s, const BatchSrc& b, const int* t, const float* sqrt_ac, const float* sqrt_1m, const float* noise_in,
                               int64_t rows, int cols, int cd, uint64_t seed, uint32_t row_offset, float* x_t, float* noise_out, int* t_out, int T,
                               float* cond_out, float* x0_out, int ldxt = 0, const ZeroList* zl = nullptr, int kind = OSD_PRED_EPSILON,
                               bool masked = false);
// q_sample of the likelihood bound's (timestep, patient) pairs (k_elem.hip: k_q_sample_pairs).  Row r of the launch is pair
// pair0 + r of a [S][n_pat] grid: patient i = pair % n_pat, timestep t_row[r] (t_row non-null) or t_list[pair / n_pat].  x0 / cond rows
// are gathered from patient i (cond_out null: no condition rows written); noise_in, if given, points at row 0 of the launch.
struct PairRows { int64_t pair0, n_pat; const int* t_row; const int* t_list; };
hipError_t launch_q_sample_pairs(hipStream_t s, const float* x0, const float* cond, int cd, const PairRows& pr, const float* sqrt_ac,
                                 const float* sqrt_1m, const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                                 int ldxt, float* target_out, int* t_out, float* cond_out, const ZeroList* zl, int kind);
// q_sample of the noise map's (level, patient) pairs (k_elem.hip: k_q_sample_map).  Row r of the launch is pair
// pair0 + r of a [n_steps - s0][n_pat] grid: patient i = pair % n_pat, level s = s0 + pair / n_pat of the plan t_list / coef [n_steps][4].
// noise_in, if given, is the CALL's [n_steps][n_pat][cols] (not the launch's first row: a row reads two levels of it).  The row's
// y_s goes to x_t (null: not written), y_{s-1} - A_s y_s to target_out and (B_s, 1 / C_s, where z_s goes) to row_out -- both only for
// s > 0 --, and y_{n_steps-1} of patient i to x_start + i * cols.
struct MapRows { int64_t pair0, n_pat; const int* t_list; const float* coef; int n_steps, s0; };
hipError_t launch_q_sample_map(hipStream_t s, const float* x0, const float* cond, int cd, const MapRows& mr, const float* sqrt_ac,
                               const float* sqrt_1m, const float* noise_in, int64_t rows, int cols, uint64_t seed, uint32_t row_offset, float* x_t,
                               int ldxt, float* target_out, MapRow* row_out, float* x_start, int* t_out, float* cond_out, const ZeroList* zl);
// classifier-free guidance on the last hidden activation: h[r] = h[m + r] + w * (h[r] - h[m + r]) for r < m, in place (h: [2 m][cols])
hipError_t launch_guide_combine(hipStream_t s, float* h, int64_t m, int cols, float w);
// condition dropout of a caller-supplied batch: out[r] = row r keeps its condition (rng.h: cond_kept) ? cond[r] : null_cond
hipError_t launch_cond_dropout(hipStream_t s, const float* cond, const float* null_cond, const float* keep, float p, int64_t rows, int cd,
                               uint64_t seed, uint32_t row_offset, float* out);
hipError_t launch_clamp_int(hipStream_t s, const int* in, int64_t n, int lo, int hi, int* out);
hipError_t launch_randint(hipStream_t s, int* out, int64_t n, int hi, uint64_t seed, uint32_t row_offset);
hipError_t launch_mixup(hipStream_t s, const float* v, const int64_t* perm, double lam, int64_t rows, int cols, float* out);
hipError_t launch_mixup3(hipStream_t s, const float* d, const float* c, const float* sv, const int64_t* perm, double lam, int64_t rows, int D,
                         int cd, float* od, float* oc, float* os);
hipError_t launch_threshold(hipStream_t s, const float* x, int ldx, int64_t rows, int cols, float thr, float* out);

}  // namespace osd
