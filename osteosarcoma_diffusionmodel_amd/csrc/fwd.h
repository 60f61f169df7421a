// fwd.h -- forward-pass and reverse-chain plumbing shared by api.hip, split.hip, train.hip and the chain kernels' host files.
#pragma once
#include <algorithm>
#include <vector>
#include "handle.h"
#include "gemm.h"
#include "kernels.h"

namespace osd {

struct TrunkIn {
  const float* x; int ldx; int64_t n;
  float* in_slabs; int in_slices; // > 1: input_proj split-K over that many slices (k_fused.hip), slabs = in_slices x n x H0 floats
  float* gn_slabs; int gn_slices; // > 1: the >= 512-deep Linear+GroupNorm layers split K over workgroups (k_fused.hip: launch_gn_silu_splitk); slabs =
                                 // (gn_slices + 1) x n x max width floats.  Eval-mode sampling of small batches only (another fp32 summation order)
  bool ksplit;                   // training-sized batches: ask for the two-wave-group GEMM variant (gemm_glds.h, NG = 2) in every layer
  bool a_unpacked;               // input_proj reads input_proj.weight itself (clamped at D, GemmArgs::a_kmax) instead of the packed copy;
                                 // x must then be zero in the columns [D, kx) (training: the library's own x_t buffer)
  int kx;                        // K extent of input_proj: 0 = D; Dp when x is the padded chain state (handle.h)
  const int* t_index;            // per-row t (training) or null
  const int* t_dev; int t_imm;   // shared t: device counter (sampling chain) or immediate
  const float* temb;             // rows a shared t reads: null = the handle's [T][H0] table (d_temb), else a chain's step plan (StepPlan)
  int64_t guide_m;               // > 0: a classifier-free-guidance step.  x holds guide_m state rows, n == 2 * guide_m: input_proj runs once over the
  const float* cproj0;           // state rows and writes h0[r] with the row's c_proj and h0[guide_m + r] with cproj0 [H0] (EpiInputGuided)
  bool input_only;               // stop after input_proj (the blocks run elsewhere: train_squad.h)
  bool train;                    // dropout active
  bool save;                     // keep pre-norm activations + GroupNorm statistics for backward
  const float* const* masks;     // injected keep-masks per block, or null -> Philox
  uint64_t seed; uint32_t row_offset; uint32_t drop_step; const int* drop_step_dev;
  int* path;                     // training calls: OSD_TP_* bits of what ran are OR-ed in (handle.h: last_train_path), else null
};

int64_t carve_fwd(const Arch& a, float* base, int64_t n, bool train, FwdWs* ws);
int run_cond(osd_handle* h, hipStream_t s, const float* cond, int64_t n, const FwdWs& ws);
int run_trunk(osd_handle* h, hipStream_t s, const FwdWs& ws, const TrunkIn& in);
int refresh_derived(osd_handle* h, hipStream_t s, bool pack_in_w = true);
int ensure_packed(osd_handle* h, hipStream_t s);
GemmArgs output_proj_args(osd_handle* h, const FwdWs& ws, int64_t n, bool padded = false);
int upload_null_cond(osd_handle* h, int slot, const float* null_cond_host, const float** dev);
int check_ready(osd_handle* h);
int check_rows(int64_t n);
// osd_set_output_link and osd_set_prediction can be called in either order: every call that uses the link refuses a type other than sample
int check_output_link(const osd_handle* h);

// ---- the per-layer chunk drivers (api.hip: chain_chunk, split.hip: split_chain_chunk) ----
// Drop the slot's previous graph once everything replayed from it has finished.
int release_graph(Slot& sl);
// S reverse steps on the slot's stream, counting sl.t_dev down from S - 1: enqueue_step() queues one step (and its own decrement) --
// S times eagerly, or once into a hipGraph (OSD_F_GRAPH) that is then replayed S times and kept in the slot until its next use.
template <class F>
int run_steps(Slot& sl, int S, int flags, F&& enqueue_step) {
  hipStream_t s = sl.stream;
  OSD_HIP(launch_set_int(s, sl.t_dev, S - 1));
  if (!(flags & OSD_F_GRAPH)) {
    for (int it = 0; it < S; ++it) OSD_TRY(enqueue_step());
    return OSD_OK;
  }
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  OSD_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue_step();
  hipError_t ce = hipStreamEndCapture(s, &graph);
  if (rc != OSD_OK) { if (graph) { hipError_t e = hipGraphDestroy(graph); (void)e; } return rc; }
  OSD_HIP(ce);
  OSD_HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  // the exec object must outlive its launches: the slot keeps it until its next use
  sl.graph.reset(graph);
  sl.exec.reset(exec);
  for (int it = 0; it < S; ++it) OSD_HIP(hipGraphLaunch(exec, s));
  return OSD_OK;
}

// chain.hip
bool chain_supported(const Arch& a);
int chain_pick_engine(osd_handle* h, int64_t n, int flags);
bool chain_uses_squad(osd_handle* h, int64_t n);
int chain_run(osd_handle* h, const ChainJob& job);
int chain_check_status(osd_handle* h);
int chain_finish(osd_handle* h, int* gave_up);
int chain_ensure_sync(osd_handle* h, int64_t n_tiles, hipStream_t s);
// ---- shared by the chunk drivers and the chain kernels' host files (api.hip) ----
// The state x [job.n][ldx] of a chain (or of one chunk of it) from job.x_T or Philox.  keep_aliased: an x_T that already is x stays
// where it is, without a launch.
int chain_init_state(osd_handle* h, hipStream_t s, const ChainJob& job, float* x, int ldx, bool keep_aliased);
// ---- host skeleton common to the three chain kernels (chain.hip) ----
// Occupancy of one kernel on one device, asked for once: resident workgroups per CU (at most `cap`) and the CU count.
struct KernelSlots { int occ = 0, cus = 0; bool ready = false; };
int kernel_slots(KernelSlots* cache, int device, const void* kernel, const void* kernel_diag, int threads, int lds_bytes, int cap, int* max_grid);
// Conditioning for all n rows, hoisted out of the chain (loop-invariant in eval mode): cw->ce1 / ce2 / cproj in the handle's
// chain_cond buffer, cproj zero-padded to rows_pad rows.
int chain_hoist_cond(osd_handle* h, hipStream_t s, const float* cond, int64_t n, int64_t rows_pad, FwdWs* cw);
// The chain state [n][state_cols], initialised from job.x_T or Philox: the caller's output rows, or -- state_cols != D -- the handle's
// padded buffer (pad columns zero), which chain_state_out copies to the output rows behind the chain's launches.
int chain_state(osd_handle* h, hipStream_t s, const ChainJob& job, int state_cols, float** xs);
int chain_state_out(hipStream_t s, const ChainJob& job, int state_cols, const float* xs);
// Steps per launch of an S-step chain: osd_set_option("chain_steps_per_launch"), or the whole chain in one launch.
inline int chain_segment_steps(const osd_handle* h, int S) { return h->chain_steps_per_launch > 0 ? h->chain_steps_per_launch : S; }
// Room for one argument block of `bytes` per launch of an S-step chain; the stream is drained first, so no earlier upload or kernel
// still reads the ring.
int chain_args_ring(osd_handle* h, hipStream_t s, int S, size_t bytes);
// Launch l's block: kept in the host ring and uploaded on s; *dev is the device copy.
int chain_args_upload(osd_handle* h, hipStream_t s, int l, const void* args, size_t bytes, const void** dev);
// fn(launch, done, n_steps) for every launch of an S-step chain
template <class F>
int for_each_segment(const osd_handle* h, int S, F&& fn) {
  const int seg = chain_segment_steps(h, S);
  int launch = 0;
  for (int done = 0; done < S; done += seg) OSD_TRY(fn(launch++, done, std::min(seg, S - done)));
  return OSD_OK;
}
// Units a workgroup runs one after the other when `grid` workgroups share n_tiles x S units (the steps of a tile are serial).
double chain_rounds(int64_t n_tiles, int S, int grid);
// A chain was launched: its status word is pending, and the host's wall-clock budget follows from the run-time estimate.
void chain_launched(osd_handle* h, double expected_ms);
// What every chain kernel's argument block says about the request: state, conditioning, plan, draws and the mutation mask.
template <class Args>
void chain_fill_request(Args& a, const osd_handle* h, const ChainJob& job, float* xs, int ld, const float* cproj) {
  a.x = xs; a.D = ld; a.n = (int)job.n;
  a.cproj = cproj; a.ldc = h->arch.H0; a.temb = job.plan.temb; a.ldt = h->arch.H0; a.coef = job.plan.coef;
  a.z = job.noises; a.ldzz = ld; a.z_step_stride = (long long)job.n * ld; a.z_t_first = job.plan.n_steps - 1;
  a.seed = job.seed; a.row_offset = (uint32_t)job.row_offset;
  a.mut_mask = job.mut_mask_out; a.mutation_dim = job.mutation_dim;
}
// chain_panel.hip
bool panel_chain_supported(const osd_handle* h);
int panel_chain_slots(osd_handle* h);
int panel_chain_pack(osd_handle* h, hipStream_t s);
int panel_chain_run(osd_handle* h, const ChainJob& job);
hipError_t launch_pack_fragments(hipStream_t s, const float* w, int ldw, int F, int K, int nfbg, int K8, float* dst);
// chain_squad.hip
bool squad_chain_supported(const osd_handle* h);
bool squad_window(osd_handle* h, int64_t n);
int squad_chain_run(osd_handle* h, const ChainJob& job);
// train_squad.h (host side in chain_squad.hip): the training forward trunk as one launch of squads
int64_t train_squad_act_floats(const Arch& a, int64_t* wpk_floats);
bool train_squad_ok(const osd_handle* h, int64_t n);
// train_squad_bwd.h: the dgrad chain (single-GPU steps, fused GroupNorm backward) as one launch of squads
struct TrainSquadBwdBufs {
  float* const* g_out; float* const* g_z2; float* const* g_mid; float* const* g_z1;      // per block, row-major (train.hip: TrainWs)
  float* g_h0;                   // dL/dh0 [n][H0]
  const float* const* masks; bool drop; uint64_t seed; uint32_t row_offset;
};
int64_t train_squad_bwd_wpk_floats(const Arch& a);
int train_squad_backward(osd_handle* h, hipStream_t s, const FwdWs& f, const TrainSquadBwdBufs& B, int64_t n, float* gact_units, float* wpk,
                         unsigned* bar_and_status, int64_t panels, float* loss_poison);
int train_squad_forward(osd_handle* h, hipStream_t s, const FwdWs& ws, const TrunkIn& in, float* act_units, float* wpk, unsigned* bar_and_status,
                        int64_t panels, float* loss_poison, float* wpk_t = nullptr);
// wgrad_group.hip
struct WgPending;
int wgrad_group_flush(osd_handle* h, hipStream_t s, int plan_index, const std::vector<WgPending>& pend, float* slabs, int64_t slab_floats,
                      int max_grid);
struct GnColItem;
int gn_colsums_flush(osd_handle* h, hipStream_t s, int plan_index, const std::vector<GnColItem>& cols);
void wgrad_group_free(osd_handle* h);
int check_row_offset(int64_t row_offset, int64_t n);
int sanitize_t(osd_handle* h, hipStream_t s, const int32_t* t_index, int64_t n, const int** out);

}  // namespace osd
