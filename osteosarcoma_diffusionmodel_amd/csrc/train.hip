// train.hip -- training entry points of the C ABI (include/osdiff.h):
// fused forward + backward of the eps-prediction MSE loss, mixup lives in api.hip,
// clip_grad_norm_ + AdamW over flat buffers.
#include <math.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <vector>
#include "handle.h"
#include "kernels.h"
#include "kernels_train.h"
#include "fwd.h"
#include "dp.h"

namespace osd {

static int t_pad(int T) { return (T + 31) / 32 * 32; }


struct TrainWs {
  FwdWs f;
  int xld;           // row stride of x_t: D, or roundup(D, 32) with zero pad columns (input_proj then reads the unpacked weight)
  float *x_t, *noise, *d_out, *u0;
  float* cond_mix;   // [n][cond_dim]: the batch's condition rows when they come from a resident dataset (osd_train_batch_source)
  float* x0_mix;     // [n][D]: the batch's data rows, only carved when the constraint losses read them
  int* t_idx;
  float *g_h0, *g_ce2, *g_ce1, *g_u, *g_temb;
  std::vector<float*> g_out, g_z2, g_mid, g_z1;
  double* normsq;
  float* partials;   // gn backward column partials
  float* slabs;      // split-K wgrad partial tiles
  int64_t slab_floats;
  float* sq_act;     // train_squad.h: unit-order activations, per 32-patient sub-panel (null: model outside the squad decomposition)
  float* sq_wpk;     // ... this step's fragment-ordered trunk weights
  float* sq_gact;    // train_squad_bwd.h: unit-order gradients, same geometry as sq_act
  float* sq_wpk_t;   // ... this step's fragment-ordered transposed weights
  unsigned* sq_bar2; // ... its barrier counters + status word
  unsigned* sq_bar;  // ... its barrier counters [panels][16] + the status word
  int64_t sq_panels;
  // constraint losses (only carved when configured)
  float *pred, *g_x0;
  ConsWs cw;
};

static int x_t_stride(const Arch& a, const ConsPlan* cp) { return (cp || a.D % 4) ? a.D : (a.D + 31) / 32 * 32; }

static int64_t carve_train(const Arch& a, float* base, int64_t n, const ConsPlan* cp, TrainWs* w) {
  int64_t off = 0;
  auto take = [&](int64_t floats) { float* p = base ? base + off : nullptr; off += up64(floats); return p; };
  float* fbase = base;
  const int64_t fwd = carve_fwd(a, fbase, n, true, &w->f);
  off = up64(fwd);
  w->xld = x_t_stride(a, cp);
  w->x_t = take(n * (int64_t)w->xld); w->noise = take(n * a.D); w->d_out = take(n * a.D);
  w->u0 = take(n * 64);
  w->cond_mix = take(n * (int64_t)a.cond_dim);
  w->t_idx = (int*)take(n);
  w->g_h0 = take(n * a.H0); w->g_ce2 = take(n * 64); w->g_ce1 = take(n * 64); w->g_u = take(n * 64);
  w->g_temb = take((int64_t)t_pad(a.T) * a.H0 + COND_BWD_PART_FLOATS);      // + k_cond_bwd's partial copies (zeroed with the table)
  w->g_out.resize(a.n_blocks); w->g_z2.resize(a.n_blocks); w->g_mid.resize(a.n_blocks); w->g_z1.resize(a.n_blocks);
  for (int b = 0; b < a.n_blocks; ++b) {
    const int64_t c = a.block_out[b];
    w->g_out[b] = take(n * c); w->g_z2[b] = take(n * c); w->g_mid[b] = take(n * c); w->g_z1[b] = take(n * c);
  }
  w->normsq = (double*)take(16);
  int cmax = 0;
  for (int c : a.block_out) cmax = c > cmax ? c : cmax;
  w->partials = take((int64_t)GN_BWD_MAX_BLOCKS * 3 * cmax);
  w->slab_floats = 16 * 1024 * 1024;      // 64 MB of split-K slabs
  w->slabs = take(w->slab_floats);
  {
    int64_t wf = 0;
    const int64_t af = train_squad_act_floats(a, &wf);
    w->sq_panels = (n + 63) / 64;
    w->sq_act = af ? take(2 * w->sq_panels * af) : nullptr;
    w->sq_wpk = af ? take(wf) : nullptr;
    w->sq_bar = af ? (unsigned*)take(w->sq_panels * 16 + 16) : nullptr;      // barrier counters | status word
    w->sq_gact = af ? take(2 * w->sq_panels * af) : nullptr;
    w->sq_wpk_t = af ? take(train_squad_bwd_wpk_floats(a)) : nullptr;
    w->sq_bar2 = af ? (unsigned*)take(w->sq_panels * 16 + 16) : nullptr;
  }
  w->pred = w->g_x0 = w->x0_mix = nullptr;
  if (cp) {
    w->pred = take(n * a.D); w->g_x0 = take(n * a.D); w->x0_mix = take(n * a.D);
    const int64_t bytes = cons_carve(*cp, n, a.D, nullptr, &w->cw);
    char* cbase = (char*)take((bytes + 3) / 4);
    cons_carve(*cp, n, a.D, cbase, &w->cw);
  }
  return off;
}

// out[p][f] = sum_k A(f,k) B(p,k) helpers for the two backward GEMM shapes
// dW[n_out][k_in] = sum_m gz[m][n_out] * x[m][k_in].  The reduction runs over the batch, the output is only
// n_out x k_in: split the batch over blockIdx.y so that ~1024 workgroups exist, each writing its partial
// tile to a slab, then sum the slabs in a fixed order (deterministic; no float atomics).
static bool small_wgrad_ok(int kin, int nout, int lddw) { return kin <= 8 && nout * kin <= 256 && lddw == kin; }

// `dbias_small`: taken by the small path only (it adds sum_m gz[m][n] into it); every other path leaves the bias to the caller
static hipError_t wgrad(hipStream_t s, const TrainWs& w, const float* x, int ldx, int kin, const float* gz, int ldg, int nout, int64_t rows, float* dw, int lddw,
                        float* dbias_small = nullptr) {
  if (small_wgrad_ok(kin, nout, lddw)) return launch_small_wgrad(s, x, kin, gz, ldg, nout, rows, dw, dbias_small);
  GemmArgs g{};
  g.A = x; g.lda = ldx; g.B0 = gz; g.ldb0 = ldg; g.K0 = (int)rows; g.F = kin; g.P = nout; g.K = (int)rows;
  const long tiles = (long)((kin + 63) / 64) * ((nout + 63) / 64);
  constexpr int WGRAD_TARGET = 512;
  int slices = (int)((WGRAD_TARGET + tiles - 1) / tiles);
  const int max_slices = (int)((rows + 127) / 128);
  if (slices > max_slices) slices = max_slices;
  const int64_t numel = (int64_t)nout * kin;
  while (slices > 1 && (int64_t)slices * numel > w.slab_floats) --slices;
  if (slices <= 1 || kin % 4 || lddw % 4 || (reinterpret_cast<uintptr_t>(dw) & 15)) return launch_linear(s, g, false, false, nullptr, dw, lddw, false, false);
  g.kchunk = (int)(((rows + slices - 1) / slices + 31) / 32 * 32);
  const int ns = (int)((rows + g.kchunk - 1) / g.kchunk);
  hipError_t e = launch_wgrad_splitk(s, g, w.slabs, kin, numel);
  if (e != hipSuccess) return e;
  return launch_slab_reduce(s, w.slabs, ns, nout, kin, numel, dw, lddw);
}
static hipError_t dgrad(hipStream_t s, const float* w, int ldw, int kin, const float* gz, int ldg, int nout, int64_t rows, float* dx, int lddx, bool accumulate) {
  // dX[m][k_in] (+)= sum_n gz[m][n] * W[n][k_in]
  GemmArgs g{};
  g.A = w; g.lda = ldw; g.B0 = gz; g.ldb0 = ldg; g.K0 = nout; g.F = kin; g.P = (int)rows; g.K = nout;
  return launch_linear(s, g, false, true, nullptr, dx, lddx, false, accumulate);
}


// sizes (and on growth re-allocates) the training arena for n rows and carves it
static int ensure_train_ws(osd_handle* h, hipStream_t s, int64_t n, const ConsPlan* cp, TrainWs* w) {
  const Arch& a = h->arch;
  const int64_t need = carve_train(a, nullptr, n, cp, w);
  h->dp_replay_ok = false;               // the workspace is about to be carved (and perhaps re-allocated) for another call
  OSD_TRY(h->train_arena.reserve(need, s));
  carve_train(a, h->train_arena, n, cp, w);
  return OSD_OK;
}

// ConditionalEmbedding + cond_proj with the pre-activation kept for backward (models/diffusion.py:101-105, 226)
// (Tried: the whole conditioning branch + the time_proj table as ONE VALU kernel instead of k_cond_mlp_fwd + two tile GEMMs of
// 7-10 us each: 49 us -- one 87 KB-LDS workgroup per CU, 1.25 rounds, no latency hiding.  Dropped.)
static int cond_embed_fwd(osd_handle* h, hipStream_t s, const float* cond, int64_t n, TrainWs& w) {
  const Arch& a = h->arch;
  const ParamMap& pm = a.pm;
  // the two 64-wide layers and the SiLU between them in one launch (k_cond_mlp_fwd), cond_proj on the tile GEMM
  OSD_HIP(launch_cond_mlp_fwd(s, cond, a.cond_dim, h->params[pm.ce0_w], h->params[pm.ce0_b], h->params[pm.ce2_w], h->params[pm.ce2_b], n,
                              w.u0, w.f.ce1, w.f.ce2));
  GemmArgs g{};
  g.A = h->params[pm.cp_w]; g.lda = 64; g.B0 = w.f.ce2; g.ldb0 = 64; g.K0 = 64; g.K = 64; g.P = (int)n; g.F = a.H0;
  OSD_HIP(launch_linear(s, g, true, true, h->params[pm.cp_b], w.f.cproj, a.H0, false, false));
  return OSD_OK;
}

static void zero_add(ZeroList* zl, float* p, int64_t c) { zl->ptr[zl->n] = p; zl->count[zl->n] = c; ++zl->n; }

// zeroes what the backward accumulates atomically (time-embedding table gradient, the small bias gradients)
static void add_backward_zeros(const Arch& a, const TrainWs& w, float* const* grads, ZeroList* zl) {
  const ParamMap& pm = a.pm;
  zero_add(zl, w.g_temb, (int64_t)t_pad(a.T) * a.H0 + COND_BWD_PART_FLOATS);
  const int small[] = {pm.ce0_b, pm.ce2_b, pm.in_b, pm.cp_b, pm.tp_b, pm.out_b};
  for (int i : small) zero_add(zl, grads[i], pm.numel[i]);
  if (small_wgrad_ok(a.cond_dim, 64, a.cond_dim)) zero_add(zl, grads[pm.ce0_w], pm.numel[pm.ce0_w]);     // k_small_wgrad adds into it
  for (const LayerDesc& l : a.layers) {          // GroupNorm backward adds its per-block column sums atomically
    zero_add(zl, grads[l.b], pm.numel[l.b]); zero_add(zl, grads[l.gamma], pm.numel[l.gamma]); zero_add(zl, grads[l.beta], pm.numel[l.beta]);
  }
}

// Does the step's dgrad chain -- everything between the first dgrad (output_proj) and the last (into h0) -- run as one launch of
// squads (train_squad_bwd.h)?  Single-GPU steps only: bucket events want the per-layer launches, whose weight gradients can
// be flushed mid-pass.  The one answer serves the forward (the transposed weights ride in its pack launch) and the backward
// (which consumes them).  train_squad_ok admits only layers of width 256 / 512 in eight groups, i.e. group widths 32 / 64 --
// exactly those of dgrad_gnbwd_supported -- so squads imply the fused GroupNorm backward; BackwardPass::run checks it.
static bool squad_backward(const osd_handle* h, int64_t n, bool want_grads, bool want_events) {
  return want_grads && !want_events && h->train_squad >= 2 && train_squad_ok(h, n);
}

// the handle's side stream (memory-bound leaves of the backward pass: GroupNorm affine gradients, small weight gradients).
// Default priority: a LOW-priority stream makes the HIP runtime open a low-priority hardware queue, and streams created later
// in the process -- e.g. the sampling slots of a model built after a training run, the reference's `--steps train generate` --
// were seen to land on it: their launch-bound hipGraph replays then ran 3.3x slower (bench.py reference_workload: 3700 -> 1130
// patients/s).  The leaves no longer need the low priority anyway: the grouped weight-gradient launch runs on the main stream.
static int side_stream(osd_handle* h, hipStream_t* out) {
  if (!h->wgrad_stream) OSD_HIP(hipStreamCreateWithFlags(h->wgrad_stream.put(), hipStreamNonBlocking));
  *out = h->wgrad_stream;
  return OSD_OK;
}

// dW[nout][kin] (row stride lddw) = sum over rows of gz[row][nout] x[row][kin], both operands dense; `bias`: a gradient equal to gz's column sums
static WgPending wg_item(const float* x, int kin, const float* gz, int nout, int64_t rows, float* dw, int lddw, float* bias = nullptr) {
  return WgPending{x, kin, kin, gz, nout, nout, rows, dw, lddw, {bias, nullptr, nullptr}};
}
// dX[n][kin] = gz[n][nout] W[nout][kin], W at row stride ldw, gz dense
struct DgradOp { const float* w; int ldw, kin; const float* gz; int nout; };
// one GroupNorm+SiLU(+dropout) layer as its backward sees it: pre-norm activations and statistics in, dL/dz and dL/dy out
struct GnLayer { const LayerDesc& l; const float* z; const float* stats; float* gz; float* gy; int blk; bool with_drop; };
// what every variant of one block's backward reads
struct Block {
  int b; const LayerDesc& l1; const LayerDesc& l2;
  int C, Kt;                // width, and input width of the first Linear (main input + skip)
  const float* xin;         // the block's main input
  float* gdst; bool acc;    // ... its gradient; an encoder output already holds its skip gradient
  int skip_block;           // the encoder block whose output is the skip input, or -1
};
struct DgradResult {        // an OSD_* code; skip_carried: the launch also produced the skip connection's share
  int rc; bool skip_carried;
  DgradResult(int rc_, bool carried = false) : rc(rc_), skip_carried(carried) {}
};

// The backward pass from dL/d eps_hat (d_out [n][D]) to every parameter gradient (and optionally dL/dx_t), over the
// activations a training-mode forward left in W.
// Two streams: the chain  GroupNorm/SiLU backward -> dgrad -> next layer  is the critical path and stays on the
// handle's stream; every weight/bias gradient (wgrad, split-K slab sums, column sums) is a leaf and goes to a
// lower-priority side stream that fills the CUs the small dgrad launches leave idle.  fork() orders the side
// stream behind what the main stream has produced so far; the side stream owns the slab workspace.
struct BackwardPass {
  osd_handle* h; const Arch& a; hipStream_t s, s2; TrainWs& W; int64_t n; float* const* grads; void* const* events;
  const float* const* masks; uint64_t seed; uint32_t roff; bool drop; float keep_scale;
  bool squads;                         // squad_backward(): the dgrad chain is one launch
  bool fuse = true;                    // GroupNorm backward inside the dgrad epilogues
  std::vector<WgPending> pend;         // weight gradients waiting for the next grouped launch
  std::vector<GnColItem> cols;         // d gamma / d beta column sums waiting for side_leaves()
  int ev = 0, ev_closed = 0;           // bucket events recorded / buckets complete up to the pending weight gradients
  int n_flush = 0, n_cols_flush = 0;   // plan slots of the grouped launches / of the column-sum lists
  size_t ev_used = 0;                  // cursor into the handle's pool of internal events
  bool s2_slabs_busy = false;          // an immediate split-K weight gradient on the side stream may still be using W.slabs
  hipEvent_t mid_done = nullptr;       // the side stream is through with the slab workspace
  // Differentially private step (osd_set_dp_clip; dp.h): the dgrad chain runs first and every leaf -- weight gradients, column sums, the
  // time-table scatter -- waits in dp_wg / cols until dp_clip_leaves() has measured each row's gradient norm and scaled the rows of
  // the buffers the leaves read.  Everything behind the dgrad chain is linear in those rows, so the scaling is exact.
  bool dp = false, dp_replay = false;
  std::vector<WgPending> dp_wg;        // the weight gradients in the order the pass met them

  BackwardPass(osd_handle* h_, hipStream_t s_, TrainWs& W_, int64_t n_, bool train, const float* const* masks_, uint64_t seed_, uint32_t roff_,
               float* const* grads_, void* const* events_, bool squads_)
      : h(h_), a(h_->arch), s(s_), s2(s_), W(W_), n(n_), grads(grads_), events(events_), masks(masks_), seed(seed_), roff(roff_),
        drop(train && h_->cfg.dropout_p > 0.f), keep_scale((float)(1.0 / (1.0 - (double)h_->cfg.dropout_p))), squads(squads_) {}

  int next_event(hipEvent_t* out) {
    if (ev_used == h->ev_pool.size()) {
      Event e;
      OSD_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
      h->ev_pool.push_back(std::move(e));
    }
    *out = h->ev_pool[ev_used++];
    return OSD_OK;
  }
  int fork() {          // side stream waits for everything enqueued on the main stream so far
    if (s2 == s) return OSD_OK;
    hipEvent_t e;
    OSD_TRY(next_event(&e));
    OSD_HIP(hipEventRecord(e, s));
    OSD_HIP(hipStreamWaitEvent(s2, e, 0));
    return OSD_OK;
  }
  int join() {          // main stream waits for everything enqueued on the side stream so far
    hipEvent_t e;
    OSD_TRY(next_event(&e));
    OSD_HIP(hipEventRecord(e, s2));
    OSD_HIP(hipStreamWaitEvent(s, e, 0));
    return OSD_OK;
  }
  // Weight gradients are leaves: they are collected and launched as ONE grouped GEMM per flush point (after the decoder +
  // bottleneck half of the backward pass, and at its end) instead of ~17 launches of a few tiles each.  A gradient bucket is
  // final once the flush that carries its weight gradients has been enqueued, so bucket events are recorded there.
  void bucket_closed() { ++ev_closed; }      // bucket complete up to the pending weight gradients
  int record_closed_buckets(hipStream_t st) {
    for (; ev < ev_closed; ++ev)
      if (events) OSD_HIP(hipEventRecord((hipEvent_t)events[ev], st));
    return OSD_OK;
  }
  // a weight gradient: deferred to the next grouped launch when eligible, else launched now on the side stream (which then
  // has to see what the main stream produced: each fork costs the main stream a few microseconds, so only then)
  // bias[0..2]: bias gradients equal to the column sums of gz (the Linear's own bias and tensors that share it); they ride along
  // with the grouped launch, with the small kernel, or -- immediate GEMM path -- take a column-sum launch
  // (Round 3 also built the whole trunk backward as ONE persistent launch -- dgrad tiles and weight-gradient items as work units
  // ordered by dependency counters.  Parity-green and slower, 800 vs 539 us: a wave streaming fp32 MFMAs starves the co-resident
  // wave's VALU epilogue, so the dgrad chain stretched.  Removed in round 4; the stamps and the verdict are profiles/r03_bwd_persist.md.)
  int weight_grad(const WgPending& wp) {
    if (dp && !dp_replay) { dp_wg.push_back(wp); return OSD_OK; }
    if (wp.kin >= 16 && wgrad_group_ok(wp)) { pend.push_back(wp); h->last_train_path |= OSD_TP_WGRAD_GROUP; return OSD_OK; }
    h->last_train_path |= OSD_TP_WGRAD_DIRECT;
    float* const b0 = wp.bias[0];
    const bool small = small_wgrad_ok(wp.kin, wp.nout, wp.lddw);
    if (small && !events) {            // a 5 us kernel whose inputs are on the main stream: run it there (no fork, no event)
      OSD_HIP(wgrad(s, W, wp.x, wp.ldx, wp.kin, wp.gz, wp.ldg, wp.nout, wp.rows, wp.dw, wp.lddw, b0));
      return OSD_OK;
    }
    OSD_TRY(fork());
    OSD_HIP(wgrad(s2, W, wp.x, wp.ldx, wp.kin, wp.gz, wp.ldg, wp.nout, wp.rows, wp.dw, wp.lddw, b0));
    if (!small && s2 != s) s2_slabs_busy = true;
    if (b0 && !small) OSD_HIP(launch_colsum(s2, wp.gz, wp.ldg, wp.rows, wp.nout, b0));
    if (b0 && small && (wp.bias[1] || wp.bias[2])) { set_error("internal: shared bias on the small weight-gradient path"); return OSD_EINVAL; }
    if (b0 && !small)
      for (float* bx : {wp.bias[1], wp.bias[2]})
        if (bx) OSD_HIP(hipMemcpyAsync(bx, b0, (size_t)wp.nout * 4, hipMemcpyDeviceToDevice, s2));
    return OSD_OK;
  }
  // d gamma / d beta of the layers whose backward ran in a dgrad epilogue: memory-bound leaves, one launch per call.  They
  // go to the side stream as soon as the block loop is through (beside the last small GEMMs of the main stream), not next to
  // the grouped weight-gradient launch, whose 512 workgroups would keep them off the CUs until it ends.
  int side_leaves(hipStream_t st) {
    if (!cols.empty()) {
      OSD_TRY(gn_colsums_flush(h, st, 8 + n_cols_flush++, cols));      // plan slots 8.. hold the column-sum lists
      cols.clear();
    }
    return OSD_OK;
  }
  // mid-pass flush (data parallel: the decoder half's buckets can go to the wire early): grouped weight gradients on the side
  // stream, one workgroup per CU walking the list so that the other slot of every CU stays with the dgrad chain of the main
  // stream (a full-width launch starved it: a 16 us dgrad took 104 us)
  int flush_mid() {
    // the events recorded behind the weight gradients must cover the affine gradients too: those go first
    if (s2 != s && !cols.empty()) OSD_TRY(fork());
    OSD_TRY(side_leaves(s2));
    OSD_TRY(fork());                  // the side stream sees every gz produced so far
    constexpr int WGRAD_MID_CAP = 256;
    OSD_TRY(wgrad_group_flush(h, s2, n_flush++, pend, W.slabs, W.slab_floats, s2 != s ? WGRAD_MID_CAP : 0));
    pend.clear();
    OSD_TRY(record_closed_buckets(s2));
    if (s2 != s) { OSD_TRY(next_event(&mid_done)); OSD_HIP(hipEventRecord(mid_done, s2)); }
    return OSD_OK;
  }
  // End-of-pass flush.  The grouped weight-gradient GEMM (the long pole, ~200 us at batch 4096) stays on the MAIN stream: no
  // stream hop in front of it or between it and the optimizer.  The memory-bound leaves run beside it on the side stream and
  // are long done when the main stream joins.
  int flush_end() {
    if (s2 != s) {
      if (!cols.empty()) { OSD_TRY(fork()); OSD_TRY(side_leaves(s2)); }
      if (mid_done) OSD_HIP(hipStreamWaitEvent(s, mid_done, 0));     // slab workspace handed back by the mid-pass flush
      if (s2_slabs_busy && !pend.empty()) {                           // ... and by immediate split-K weight gradients (e.g. the
        OSD_TRY(join());                                              // ConditionalEmbedding's first Linear at cond_dim 8 or 12)
        s2_slabs_busy = false;
      }
    } else {
      OSD_TRY(side_leaves(s));
    }
    OSD_TRY(wgrad_group_flush(h, s, n_flush++, pend, W.slabs, W.slab_floats, 0));
    pend.clear();
    if (s2 != s) OSD_TRY(join());
    return record_closed_buckets(s);
  }

  GnLayer gn_layer(int b, int half) const {      // half 0: the block's first Linear (dropout sits behind it), 1: its second
    if (half) return GnLayer{a.layers[2 * b + 1], W.f.z2[b], W.f.st2[b], W.g_z2[b], W.g_out[b], b, false};
    return GnLayer{a.layers[2 * b], W.f.z1[b], W.f.st1[b], W.g_z1[b], W.g_mid[b], b, drop};
  }
  // this layer's d gamma / d beta column sums, from the dL/dy and z that a dgrad epilogue (or the squad launch) has left
  void queue_colsums(const GnLayer& t, int C) {
    cols.push_back({t.gy, C, t.z, C, t.stats, C, t.l.gw, n, grads[t.l.gamma], grads[t.l.beta]});
  }
  // dgrad whose epilogue is the GroupNorm+SiLU(+dropout) backward of `t` (z / stats of that layer): writes dL/dz and dL/dy.
  // `skip`: the skip connection's share of the same gz (plain dX = gz W_skip into out_skip) rides in the same launch where the
  // dual kernel takes the shapes.
  DgradResult dgrad_gnbwd(const DgradOp& op, const GnLayer& t, bool accumulate, const DgradOp* skip = nullptr, float* out_skip = nullptr) {
    GemmArgs g{};
    g.A = op.w; g.lda = op.ldw; g.B0 = op.gz; g.ldb0 = op.nout; g.K0 = op.nout; g.F = op.kin; g.P = (int)n; g.K = op.nout;
    g.ksplit = 1;                          // launch.h: two wave groups where a launch has ~one tile per CU and >= 32 K tiles (the first dgrad)
    GnBwdEpi e{};
    e.z = t.z; e.ldz = op.kin; e.stats = t.stats; e.gamma = h->params[t.l.gamma]; e.beta = h->params[t.l.beta];
    e.gz = t.gz; e.ldg = op.kin; e.gy = t.gy; e.ldy = op.kin; e.accumulate = accumulate ? 1 : 0;
    e.drop_mode = t.with_drop ? (masks ? 1 : 2) : 0;
    e.mask = (t.with_drop && masks) ? masks[t.blk] : nullptr; e.ldm = op.kin; e.keep_scale = keep_scale; e.p_drop = h->cfg.dropout_p;
    e.seed = seed; e.row_offset = roff; e.step = 0; e.tag = TAG_DROPOUT + (uint32_t)t.blk;
    bool carried = false;
    if (skip) {
      GemmArgs g2{};
      g2.A = skip->w; g2.lda = skip->ldw; g2.B0 = skip->gz; g2.ldb0 = skip->nout; g2.K0 = skip->nout; g2.F = skip->kin; g2.P = (int)n; g2.K = skip->nout;
      const hipError_t de = launch_dgrad_gnbwd_dual(s, g, t.l.gw, e, g2, out_skip, skip->kin);
      if (de == hipSuccess) { carried = true; h->last_train_path |= OSD_TP_DUAL_DGRAD; }
      else if (de != hipErrorInvalidValue) OSD_HIP(de);
      else (void)hipGetLastError();
    }
    if (!carried) OSD_HIP(launch_dgrad_gnbwd(s, g, t.l.gw, e));
    queue_colsums(t, op.kin);
    return DgradResult(OSD_OK, carried);
  }
  int dgrad_plain(const DgradOp& op, float* dx, bool accumulate = false) {      // dX (+)= gz W, no epilogue
    OSD_HIP(dgrad(s, op.w, op.ldw, op.kin, op.gz, op.nout, op.nout, n, dx, op.kin, accumulate));
    return OSD_OK;
  }

  // output_proj: its weight gradient, the first dgrad, and -- squads -- every dgrad between that one and the last (into h0) in one launch
  int head(const float* d_out, float* loss_poison) {
    const ParamMap& pm = a.pm;
    const int last = a.n_blocks - 1, Hl = a.block_out[last], D = a.D;
    OSD_TRY(weight_grad(wg_item(W.f.out[last], Hl, d_out, D, n, grads[pm.out_w], Hl, grads[pm.out_b])));
    bucket_closed();
    const DgradOp op{h->params[pm.out_w], Hl, Hl, d_out, D};
    if (!fuse) return dgrad_plain(op, W.g_out[last]);
    OSD_TRY(dgrad_gnbwd(op, gn_layer(last, 1), false).rc);
    if (squads) {
      TrainSquadBwdBufs B{W.g_out.data(), W.g_z2.data(), W.g_mid.data(), W.g_z1.data(), W.g_h0, masks, drop, seed, roff};
      OSD_TRY(train_squad_backward(h, s, W.f, B, n, W.sq_gact, W.sq_wpk_t, W.sq_bar2, W.sq_panels, loss_poison));
    }
    return OSD_OK;
  }
  Block block(int b) const {
    const LayerDesc& l1 = a.layers[2 * b];
    return Block{b, l1, a.layers[2 * b + 1], l1.N, l1.K1 + l1.K2, b == 0 ? W.f.h0 : W.f.out[b - 1], b == 0 ? W.g_h0 : W.g_out[b - 1],
                 (b >= 1) && (b - 1 < a.n_enc), l1.K2 > 0 ? a.skip_of(b) : -1};
  }
  // The first Linear's weight gradient (main input, skip share) closes the block's bucket.  Data parallel: once the decoder blocks
  // and the bottleneck are through, the first half of the weight gradients goes out.  Both variants of a block come through
  // here between dL/dz of the first half and the dgrads into the block's inputs.
  int first_linear_wgrads(const Block& B, float* dbias) {
    const LayerDesc& l1 = B.l1;
    OSD_TRY(weight_grad(wg_item(B.xin, l1.K1, W.g_z1[B.b], B.C, n, grads[l1.w], B.Kt, dbias)));
    if (l1.K2 > 0) OSD_TRY(weight_grad(wg_item(W.f.out[B.skip_block], l1.K2, W.g_z1[B.b], B.C, n, grads[l1.w] + l1.K1, B.Kt)));
    bucket_closed();
    if (B.b == a.n_enc && events) OSD_TRY(flush_mid());
    return OSD_OK;
  }
  // One block, GroupNorm backward in the dgrad epilogues (group widths 32 / 64).  dL/dz of the second half is in g_z2[b] (left by
  // the dgrad above it); bias gradients ride with the weight gradients.  Squads: their launch has produced every dgrad result
  // of the chain, only the column sums are left to queue (a block with a skip input is never block 0 there).
  int block_fused(const Block& B) {
    const int b = B.b, C = B.C;
    const LayerDesc& l1 = B.l1;
    OSD_TRY(weight_grad(wg_item(W.f.mid[b], C, W.g_z2[b], C, n, grads[B.l2.w], C, grads[B.l2.b])));
    if (squads) queue_colsums(gn_layer(b, 0), C);
    else OSD_TRY(dgrad_gnbwd(DgradOp{h->params[B.l2.w], C, C, W.g_z2[b], C}, gn_layer(b, 0), false).rc);
    OSD_TRY(first_linear_wgrads(B, grads[l1.b]));
    if (squads) {
      if (b > 0) queue_colsums(gn_layer(b - 1, 1), l1.K1);
      return OSD_OK;
    }
    const DgradOp main{h->params[l1.w], B.Kt, l1.K1, W.g_z1[b], C}, skip{h->params[l1.w] + l1.K1, B.Kt, l1.K2, W.g_z1[b], C};
    bool skip_open = l1.K2 > 0;
    if (b == 0) {
      OSD_TRY(dgrad_plain(main, B.gdst));
    } else {
      // into the layer that produced this block's main input; an encoder output already holds its skip gradient (written by
      // the decoder block that popped it): second dependency
      const DgradResult r = dgrad_gnbwd(main, gn_layer(b - 1, 1), B.acc, skip_open ? &skip : nullptr, skip_open ? W.g_out[B.skip_block] : nullptr);
      OSD_TRY(r.rc);
      if (r.skip_carried) skip_open = false;
    }
    if (skip_open) OSD_TRY(dgrad_plain(skip, W.g_out[B.skip_block]));
    return OSD_OK;
  }
  GnBwdArgs gn_bwd_args(const GnLayer& t, int C, bool first_half) const {
    GnBwdArgs ga{};
    ga.g = t.gy; ga.z = t.z; ga.stats = t.stats; ga.gamma = h->params[t.l.gamma]; ga.beta = h->params[t.l.beta];
    ga.gz = t.gz; ga.dgamma = grads[t.l.gamma]; ga.dbeta = grads[t.l.beta]; ga.dbias = grads[t.l.b];
    ga.rows = n; ga.C = C; ga.partials = W.partials; ga.atomic_cols = 0;      // fixed-order partial reduce: deterministic
    if (first_half) {                     // dropout sits behind it
      ga.drop_mode = drop ? (masks ? 1 : 2) : 0;
      ga.mask = (drop && masks) ? masks[t.blk] : nullptr; ga.keep_scale = keep_scale; ga.p_drop = h->cfg.dropout_p;
      ga.seed = seed; ga.row_offset = roff; ga.step = 0; ga.tag = TAG_DROPOUT + (uint32_t)t.blk;
    }
    return ga;
  }
  // One block, GroupNorm backward as its own pass between the GEMMs (other group widths); it produces the bias gradients too
  int block_gn_standalone(const Block& B) {
    const int b = B.b, C = B.C;
    const LayerDesc& l1 = B.l1;
    // second half: GroupNorm+SiLU backward, wgrad, dgrad
    OSD_HIP(launch_gn_silu_bwd(s, B.l2.gw, gn_bwd_args(gn_layer(b, 1), C, false)));
    OSD_TRY(weight_grad(wg_item(W.f.mid[b], C, W.g_z2[b], C, n, grads[B.l2.w], C)));
    OSD_TRY(dgrad_plain(DgradOp{h->params[B.l2.w], C, C, W.g_z2[b], C}, W.g_mid[b]));
    // first half
    OSD_HIP(launch_gn_silu_bwd(s, l1.gw, gn_bwd_args(gn_layer(b, 0), C, true)));
    OSD_TRY(first_linear_wgrads(B, nullptr));
    // dgrad into the producer of the main input, and into the skip input
    OSD_TRY(dgrad_plain(DgradOp{h->params[l1.w], B.Kt, l1.K1, W.g_z1[b], C}, B.gdst, B.acc));
    if (l1.K2 > 0) OSD_TRY(dgrad_plain(DgradOp{h->params[l1.w] + l1.K1, B.Kt, l1.K2, W.g_z1[b], C}, W.g_out[B.skip_block]));
    return OSD_OK;
  }
  // input_proj, time_proj, cond_proj, ConditionalEmbedding  (h0 = x W^T + b + t_emb[t] + c_proj)
  // h0 = x W^T + b_in + (t_emb W_t^T + b_t)[t] + (c W_c^T + b_c): the three biases share one gradient, the column sums of g_h0
  // (Tried: the conditioning branch's backward -- five dependent launches of 5-13 us -- and the affine-gradient column sums on the
  // side stream BESIDE the grouped weight-gradient launch instead of in front of it.  The grouped launch's older waves starve
  // them: k_gn_colsums took 202 us instead of 44 and the side chain ended after the main one -- 1042 vs 988 us per step.  Dropped.)
  int stem(const float* x_t, int x_ld, const int* t_idx, const float* cond, float* dx_t) {
    const ParamMap& pm = a.pm;
    const int D = a.D, H0 = a.H0;
    if (!dp && s2 != s && !cols.empty()) { OSD_TRY(fork()); OSD_TRY(side_leaves(s2)); }      // every GroupNorm layer's gy / z is final
    if (dx_t) OSD_TRY(dgrad_plain(DgradOp{h->params[pm.in_w], D, D, W.g_h0, H0}, dx_t));
    WgPending in = wg_item(x_t, D, W.g_h0, H0, n, grads[pm.in_w], D, grads[pm.in_b]);
    in.ldx = x_ld; in.bias[1] = grads[pm.cp_b]; in.bias[2] = grads[pm.tp_b];
    OSD_TRY(weight_grad(in));
    OSD_TRY(weight_grad(wg_item(W.f.ce2, 64, W.g_h0, H0, n, grads[pm.cp_w], 64)));
    // the branch below h0 (scatter into the time table, cond_proj's and the second embedding Linear's dgrads, SiLU backward): one launch
    // (a differentially private step takes the unfused branch: the fused launch scatters into the time table and can carry a weight
    // gradient, both leaves, before any clip factor exists; its scatter waits for dp_clip_leaves())
    const bool cond_fused = !dp && h->cond_bwd_fused && cond_bwd_ok(H0, W.g_h0, W.u0, W.g_ce2, W.g_u);
    // ... and, where the first embedding Linear has at most four inputs (k_small_wgrad's case), its weight gradient rides along
    const bool ce0_fused = cond_fused && a.cond_dim <= 4 && small_wgrad_ok(a.cond_dim, 64, a.cond_dim);
    if (cond_fused) h->last_train_path |= OSD_TP_COND_BWD;
    if (ce0_fused) h->last_train_path |= OSD_TP_COND_BWD_CE0;
    if (cond_fused) {
      OSD_HIP(launch_cond_bwd(s, W.g_h0, H0, t_idx, W.g_temb, h->params[pm.cp_w], h->params[pm.ce2_w], W.u0, n, W.g_ce2, W.g_u,
                              ce0_fused ? cond : nullptr, a.cond_dim, W.g_temb + (int64_t)t_pad(a.T) * H0, grads[pm.ce0_w], grads[pm.ce0_b]));
    } else {
      if (!dp) OSD_HIP(launch_scatter_rows(s, W.g_h0, t_idx, n, H0, W.g_temb));
      OSD_TRY(dgrad_plain(DgradOp{h->params[pm.cp_w], 64, 64, W.g_h0, H0}, W.g_ce2));
    }
    // both tables carry zero rows up to a multiple of 32 (whole K steps of the grouped kernel): they add nothing
    OSD_TRY(weight_grad(wg_item(h->d_time_emb, a.time_dim, W.g_temb, H0, t_pad(a.T), grads[pm.tp_w], a.time_dim)));
    OSD_TRY(weight_grad(wg_item(W.f.ce1, 64, W.g_ce2, 64, n, grads[pm.ce2_w], 64, grads[pm.ce2_b])));
    if (!cond_fused) {
      OSD_TRY(dgrad_plain(DgradOp{h->params[pm.ce2_w], 64, 64, W.g_ce2, 64}, W.g_ce1));
      OSD_HIP(launch_silu_bwd(s, W.u0, W.g_ce1, W.g_u, n * 64));
    }
    if (!ce0_fused) OSD_TRY(weight_grad(wg_item(cond, a.cond_dim, W.g_u, 64, n, grads[pm.ce0_w], a.cond_dim, grads[pm.ce0_b])));
    bucket_closed();
    return OSD_OK;
  }

  // The per-row norms (dp.h: one term per Linear and per GroupNorm layer, from the buffers the dgrad chain has just left), the clip factors
  // and the scaling of every buffer a leaf reads, then the leaves themselves in the order the pass met them.
  int dp_clip_leaves(const float* x_t, int x_ld, const int* t_idx, const float* cond, const float* d_out) {
    std::vector<DpNormItem> ni;
    std::vector<DpScaleItem> si;
    auto linear = [&](const float* x0, int ld0, int k0, const float* x1, int k1, const float* d, int nd) {
      DpNormItem it;
      memset(&it, 0, sizeof(it));
      it.kind = 0; it.x[0] = x0; it.ldx[0] = ld0; it.k[0] = k0; it.x[1] = x1; it.ldx[1] = k1; it.k[1] = k1;
      it.nbias = 1.f; it.d = d; it.ldd = nd; it.nd = nd;
      ni.push_back(it);
    };
    auto scaled = [&](float* p, int cols) {
      DpScaleItem it;
      memset(&it, 0, sizeof(it));
      it.p = p; it.ld = cols; it.cols = cols;
      si.push_back(it);
    };
    const int last = a.n_blocks - 1;
    linear(W.f.out[last], a.block_out[last], a.block_out[last], nullptr, 0, d_out, a.D);      // output_proj
    scaled(const_cast<float*>(d_out), a.D);
    for (int b = a.n_blocks - 1; b >= 0; --b) {
      const Block B = block(b);
      linear(W.f.mid[b], B.C, B.C, nullptr, 0, W.g_z2[b], B.C);                                // the block's second Linear
      linear(B.xin, B.l1.K1, B.l1.K1, B.l1.K2 > 0 ? W.f.out[B.skip_block] : nullptr, B.l1.K2, W.g_z1[b], B.C);      // its first: main input + skip
      for (int half = 0; half < 2; ++half) {
        const GnLayer t = gn_layer(b, half);
        DpNormItem it;
        memset(&it, 0, sizeof(it));
        it.kind = 1; it.d = t.gy; it.ldd = B.C; it.nd = B.C; it.z = t.z; it.stats = t.stats; it.gw = t.l.gw;
        ni.push_back(it);
      }
      scaled(W.g_z2[b], B.C); scaled(W.g_z1[b], B.C); scaled(W.g_out[b], B.C); scaled(W.g_mid[b], B.C);
    }
    {
      // h0 = input_proj(x_t) + cond_proj(ce2) + time_proj(temb[t]): three Linears on one output gradient, each with a bias of its own
      DpNormItem it;
      memset(&it, 0, sizeof(it));
      it.kind = 0; it.x[0] = x_t; it.ldx[0] = x_ld; it.k[0] = a.D; it.x[1] = W.f.ce2; it.ldx[1] = 64; it.k[1] = 64;
      it.x[2] = h->d_time_emb; it.ldx[2] = a.time_dim; it.k[2] = a.time_dim; it.gathered = 1;      // rows t_idx[r]: a launch argument
      it.nbias = 3.f; it.d = W.g_h0; it.ldd = a.H0; it.nd = a.H0;
      ni.push_back(it);
    }
    linear(W.f.ce1, 64, 64, nullptr, 0, W.g_ce2, 64);                   // ConditionalEmbedding's second Linear
    linear(nullptr, a.cond_dim, a.cond_dim, nullptr, 0, W.g_u, 64);     // ... and its first, on the batch's conditions: a launch argument
    ni.back().x0_is_cond = 1;
    scaled(W.g_h0, a.H0); scaled(W.g_ce2, 64); scaled(W.g_u, 64);
    // the stored gradients carry the 1/n of the mean over rows (loss_scale is 1 here): a row's own norm is n times what they give
    OSD_TRY(dp_clip_rows(h, s, ni, si, n, (double)n, cond, t_idx));
    OSD_HIP(launch_scatter_rows(s, W.g_h0, t_idx, n, a.H0, W.g_temb));
    dp_replay = true;
    for (const WgPending& wp : dp_wg) OSD_TRY(weight_grad(wp));
    dp_wg.clear();
    return OSD_OK;
  }

  int run(const float* x_t, int x_ld, const int* t_idx, const float* cond, const float* d_out, float* dx_t, float* loss_poison) {
    if (h->train_streams == 2) OSD_TRY(side_stream(h, &s2));
    for (const LayerDesc& l : a.layers) fuse = fuse && dgrad_gnbwd_supported(l.gw);
    if (squads && !fuse) { set_error("internal: squad backward without the fused GroupNorm backward"); return OSD_EINVAL; }
    if (dp && !fuse) { set_error("internal: per-row clip without the fused GroupNorm backward"); return OSD_EINVAL; }
    if (dp) h->last_train_path |= OSD_TP_DP_CLIP;
    if (fuse) h->last_train_path |= OSD_TP_FUSED_GN_BWD;
    if (squads) h->last_train_path |= OSD_TP_SQUAD_BWD;
    OSD_TRY(head(d_out, loss_poison));
    for (int b = a.n_blocks - 1; b >= 0; --b) OSD_TRY(fuse ? block_fused(block(b)) : block_gn_standalone(block(b)));
    // Data parallel (bucket events requested): the encoder blocks' weight gradients go out NOW, in a grouped launch of their own, so
    // that their buckets' events fire one launch before the end of the pass -- what stays behind the last launch, and so cannot
    // overlap with any compute of this step, is the final bucket alone (input_proj + the conditioning branch: 2.1 MB of the 10.66 MB
    // instead of 5.2 MB).  Two grouped launches of ~250 items each fill the machine less well than one of 500 (the work-item list
    // is re-cut to the launch, wgrad_group.hip), so a single process keeps the one launch.
    if (events) OSD_TRY(flush_end());
    OSD_TRY(stem(x_t, x_ld, t_idx, cond, dx_t));
    if (dp) OSD_TRY(dp_clip_leaves(x_t, x_ld, t_idx, cond, d_out));
    return flush_end();          // ends with the side stream joined: the caller's stream owns every result again
  }
};

// What the entry points that touch the training workspace share around their own argument checks; each calls the pieces in its own order.
struct TrainCall {
  osd_handle* h; int64_t n; int flags;
  hipStream_t s = nullptr;
  const int* t_idx = nullptr;          // the caller's t_index clamped into [0, T), or null when none was given

  int begin(bool reset_path) {
    OSD_TRY(check_ready(h));
    if (reset_path) h->last_train_path = 0;
    return check_rows(n);
  }
  int check_outputs(void* const* events, int n_events, float* const* grads) const {      // grads may be null (loss only)
    const int n_buckets = h->arch.n_blocks + 2;
    if (events && n_events != n_buckets) { set_error("expected %d events (osd_grad_buckets), got %d", n_buckets, n_events); return OSD_EINVAL; }
    for (int i = 0; grads && i < h->arch.pm.n_params; ++i)
      if (!grads[i]) { set_error("grads[%d] is null", i); return OSD_EINVAL; }
    return OSD_OK;
  }
  int enter() {
    OSD_HIP(hipSetDevice(h->cfg.device));
    s = h->stream;
    return OSD_OK;
  }
  int timesteps(const int32_t* t_index) { return sanitize_t(h, s, t_index, n, &t_idx); }
  bool train_mode() const { return (flags & OSD_F_TRAIN_MODE) != 0; }
  int finish() const {
    if (flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(s));
    return OSD_OK;
  }
};

// "bf16 pipe if precision == 1 and the launcher accepts, else the fp32 launcher" for output_proj + loss (EpiMse or EpiLoss)
template <class Args>
static hipError_t launch_on_b3t_or_fp32(osd_handle* h, hipStream_t s, const GemmArgs& g, const Args& ea,
                                        hipError_t (*b3t)(hipStream_t, const GemmArgs&, const Args&),
                                        hipError_t (*fp32)(hipStream_t, const GemmArgs&, const Args&)) {
  // precision = 1: output_proj + loss on the bf16 matrix pipe, operands split where they are staged (gemm_b3t.h)
  hipError_t e = h->precision == 1 ? b3t(s, g, ea) : hipErrorInvalidValue;
  if (e == hipSuccess) h->last_train_path |= OSD_TP_MSE_BF16;
  if (e == hipErrorInvalidValue) { (void)hipGetLastError(); e = fp32(s, g, ea); }
  return e;
}

// One osd_train_loss_fwd_bwd call past its argument checks: zero list, forward, loss, constraint terms, backward.
struct LossStep {
  TrainCall& tc; osd_handle* h; const Arch& a; hipStream_t s; int64_t n;
  const float* x0; const float* cond; const float* noise; const float* const* masks; uint64_t seed; uint32_t roff;
  float* loss_out; float* const* grads; double loss_scale; void* const* events;
  bool from_src, cond_drop;            // the handle's one-shots (osd_train_batch_source, osd_train_condition_dropout), consumed by this call
  bool use_pw = false, use_me = false; const ConsPlan* cp = nullptr;
  bool squads_bwd = false;             // squad_backward()
  // the likelihood bound's row mode (osd_row_sq_error / osd_bound_sweep): the rows are (timestep, patient) pairs gathered by q_sample,
  // loss() takes the per-row epilogue and writes se_out [n]; loss_out is then the squads' poison word, not a loss
  const PairRows* pairs = nullptr; float* se_out = nullptr;
  // the noise map (osd_noise_map): the rows are (level, patient) pairs of a step plan, `noise` is the CALL's [n_steps][n_pat][D], loss()
  // takes EpiNoiseMap and writes z_out (the call's noises_out); the rows' records live where dL/dout would (w.d_out: never written without grads)
  const MapRows* map = nullptr; float* z_out = nullptr; float* x_start = nullptr;
  TrainWs w;

  // everything that is accumulated atomically must start at zero: zeroed by the q_sample kernel's own grid
  int zero_list(ZeroList* zl) {
    zero_add(zl, loss_out, 1);
    if (w.sq_bar && train_squad_ok(h, n) && !map) {      // the squads' barrier counters + status words (forward, backward)
      zero_add(zl, reinterpret_cast<float*>(w.sq_bar), w.sq_panels * 16 + 16);
      zero_add(zl, reinterpret_cast<float*>(w.sq_bar2), w.sq_panels * 16 + 16);
    }
    if (cp) zero_add(zl, h->parts_dev, 3);
    if (cp && grads) zero_add(zl, w.g_x0, n * (int64_t)a.D);
    if (grads) add_backward_zeros(a, w, grads, zl);
    if (zl->n > 128) { set_error("too many parameter tensors"); return OSD_EUNSUPPORTED; }
    return OSD_OK;
  }
  // q_sample (with the gather + mixup of a resident batch, the draw of t and the zeroing) and condition dropout
  int noised_batch(const ZeroList& zl) {
    const int D = a.D;
    // t ~ randint(0, T) is drawn inside q_sample (one launch less) and kept in w.t_idx for the layers that gather by it
    int* t_draw = nullptr;
    if (!tc.t_idx) { t_draw = w.t_idx; tc.t_idx = w.t_idx; }
    const int* t_idx = tc.t_idx;
    if (map) {      // ahead of everything that follows the prediction type or the mask: the plan's (A, B) carry the type, the map ignores the mask
      OSD_HIP(launch_q_sample_map(s, x0, cond, a.cond_dim, *map, h->d_sqrt_ac, h->d_sqrt_1m, noise, n, D, seed, roff, w.x_t, w.xld, w.noise,
                                  reinterpret_cast<MapRow*>(w.d_out), x_start, w.t_idx, w.cond_mix, &zl));
      cond = w.cond_mix;
      tc.t_idx = w.t_idx;
      return OSD_OK;
    }
    // a non-eps target (osd_set_prediction) is formed by the same pass and lands in w.noise, injected noise or not
    if (h->pred_type != OSD_PRED_EPSILON) h->last_train_path |= OSD_TP_TARGET;
    // osd_set_loss_mask: NaN in x0 = not observed; the target always lands in w.noise, NaN-marked (the row mode was refused before)
    const bool masked = h->loss_mask;
    if (masked) h->last_train_path |= OSD_TP_MASKED;
    if (se_out) {
      PairRows pr = *pairs;
      pr.t_row = t_draw ? nullptr : t_idx;          // the caller's per-row timesteps (clamped), else the sweep's list
      const bool gather = pr.t_row == nullptr;      // a sweep's rows name patients: their conditions land in the workspace
      const bool own_target = noise && h->pred_type == OSD_PRED_EPSILON;
      OSD_HIP(launch_q_sample_pairs(s, x0, cond, a.cond_dim, pr, h->d_sqrt_ac, h->d_sqrt_1m, noise, n, D, seed, roff, w.x_t, w.xld,
                                    own_target ? nullptr : w.noise, w.t_idx, gather ? w.cond_mix : nullptr, &zl, h->pred_type));
      if (gather) cond = w.cond_mix;
      tc.t_idx = w.t_idx;
      return OSD_OK;
    }
    if (from_src) {
      // rows gathered from the resident dataset, mixed up and noised in one pass; conditions land in the workspace
      OSD_HIP(launch_q_sample_src(s, h->batch_src, t_draw ? nullptr : t_idx, h->d_sqrt_ac, h->d_sqrt_1m, noise, n, D, a.cond_dim, seed, roff, w.x_t,
                                  w.noise, t_draw, a.T, w.cond_mix, cp ? w.x0_mix : nullptr, w.xld, &zl, h->pred_type, masked));
      cond = w.cond_mix;
      x0 = cp ? w.x0_mix : nullptr;
      // condition dropout after the mix: the null condition into the rows that drop theirs, in place (one tiny launch, only when asked for)
      if (cond_drop)
        OSD_HIP(launch_cond_dropout(s, w.cond_mix, h->null_cond.dev() + up64(a.cond_dim), h->cond_drop_keep, h->cond_drop_p, n,
                                    a.cond_dim, seed, roff, w.cond_mix));
    } else {
      OSD_HIP(launch_q_sample(s, x0, t_draw ? nullptr : t_idx, h->d_sqrt_ac, h->d_sqrt_1m, noise, n, D, seed, roff, w.x_t, w.noise, t_draw, a.T, w.xld, &zl,
                              h->pred_type, masked));
      if (cond_drop) {       // condition dropout of a caller-supplied batch: the replaced rows land in the workspace
        OSD_HIP(launch_cond_dropout(s, cond, h->null_cond.dev() + up64(a.cond_dim), h->cond_drop_keep, h->cond_drop_p, n, a.cond_dim,
                                    seed, roff, w.cond_mix));
        cond = w.cond_mix;
      }
    }
    return OSD_OK;
  }
  // forward (models/diffusion.py:361-377) up to the last block's output
  int forward(const int32_t* t_index) {
    const int D = a.D;
    ZeroList zl{};
    OSD_TRY(zero_list(&zl));
    // x_t rows are padded to whole K steps with zeros when nothing else reads them with the dense stride: input_proj then takes
    // input_proj.weight as it is (clamped at D) and the per-step packed copy of that weight is not made
    const bool unpacked = w.xld > D;
    if (unpacked) h->last_train_path |= OSD_TP_X_PADDED;
    // the t_emb table (and, unless input_proj reads the weight itself, its padded copy) follow the current parameters
    OSD_TRY(refresh_derived(h, s, !unpacked));
    OSD_TRY(tc.timesteps(t_index));
    OSD_TRY(noised_batch(zl));
    OSD_TRY(cond_embed_fwd(h, s, cond, n, w));
    TrunkIn in{};
    in.x = w.x_t; in.ldx = w.xld; in.kx = unpacked ? w.xld : D; in.a_unpacked = unpacked; in.ksplit = !map;
    in.n = n; in.t_index = tc.t_idx; in.train = tc.train_mode(); in.save = grads != nullptr;
    in.masks = masks; in.seed = seed; in.row_offset = roff; in.drop_step = 0; in.path = &h->last_train_path;
    // the noise map promises a row the same bits in every launch group: neither the two-wave-group K split nor the squads, whose use
    // (and summation order) follows the row count -- the layers of the per-layer sampler at input_splitk 0
    if (map || !(w.sq_act && train_squad_ok(h, n))) return run_trunk(h, s, w.f, in);
    h->last_train_path |= OSD_TP_SQUAD_FWD;
    in.input_only = true;
    OSD_TRY(run_trunk(h, s, w.f, in));
    // the step's backward as squads as well: both weight repacks in the forward's launch
    return train_squad_forward(h, s, w.f, in, w.sq_act, w.sq_wpk, w.sq_bar, w.sq_panels, loss_out, squads_bwd ? w.sq_wpk_t : nullptr);
  }
  // output_proj + loss + dL/d eps_hat in one launch
  int loss() {
    const int D = a.D;
    const double count = (double)n * (double)D;
    GemmArgs g = output_proj_args(h, w.f, n);
    if (map) {
      EpiNoiseMap::Args em{};
      em.bias = h->params[a.pm.out_b]; em.target = w.noise; em.ldn = D;
      em.row = reinterpret_cast<const MapRow*>(w.d_out); em.z = z_out;
      OSD_HIP(launch_noise_map(s, g, em));
      return OSD_OK;
    }
    if (se_out) {
      // the slot partials take the place of dL/d eps_hat, which a call without gradients never writes: ceil(D / 64) x n <= n x D floats
      EpiRowSq::Args er{};
      er.bias = h->params[a.pm.out_b]; er.target = noise && h->pred_type == OSD_PRED_EPSILON ? noise : w.noise; er.ldn = D;
      er.part = w.d_out; er.ld = n;
      OSD_HIP(launch_row_sq(s, g, er, loss_out, se_out));
      return OSD_OK;
    }
    EpiMse::Args ea{};
    ea.bias = h->params[a.pm.out_b]; ea.noise = noise && h->pred_type == OSD_PRED_EPSILON ? noise : w.noise; ea.ldn = D;
    ea.dout = grads ? w.d_out : nullptr; ea.ldd = D; ea.pred = cp ? w.pred : nullptr; ea.ldp = D; ea.loss = loss_out;
    ea.inv_count = (float)(1.0 / count);
    if (h->n_link > 0) {
      // osd_set_output_link: cross-entropy on the logits in columns [0, n_link), the configured kind elsewhere, on EpiLossT<true, true>
      // -- the masked form as well: a NaN of the target (osd_set_loss_mask marked it) stays out.  The target is x0 in w.noise (the type
      // is sample); gscale carries l2's folded 2, which the link columns take out again.  The fp32 launcher only, whatever the precision
      ea.noise = w.noise; ea.pred = nullptr;
      ea.gscale = (float)((h->loss_kind == OSD_LOSS_L2 ? 2.0 : 1.0) * (double)loss_scale / count);
      EpiLossT<true, true>::Args ek{};
      ek.m = ea; ek.tw = h->loss_tw_set ? h->loss_tw : nullptr; ek.t_index = tc.t_idx; ek.kind = h->loss_kind; ek.delta = h->loss_delta;
      ek.n_link = h->n_link;
      h->last_train_path |= OSD_TP_LOSS_EPI | OSD_TP_LINK;
      OSD_HIP(launch_loss_link(s, g, ek));
      return OSD_OK;
    }
    if (h->loss_mask) {
      // osd_set_loss_mask: every kind (the default l2 without a table included) on EpiLossT<true>, against the NaN-marked target in
      // w.noise whoever supplied eps; the fp32 launcher only, whatever the precision
      ea.noise = w.noise; ea.pred = nullptr;
      ea.gscale = (float)((h->loss_kind == OSD_LOSS_L2 ? 2.0 : 1.0) * (double)loss_scale / count);
      EpiLossT<true>::Args em{};
      em.m = ea; em.tw = h->loss_tw_set ? h->loss_tw : nullptr; em.t_index = tc.t_idx; em.kind = h->loss_kind; em.delta = h->loss_delta;
      h->last_train_path |= OSD_TP_LOSS_EPI;
      OSD_HIP(launch_loss_masked(s, g, em));
      return OSD_OK;
    }
    if (h->loss_kind == OSD_LOSS_L2 && !h->loss_tw_set) {
      ea.gscale = (float)(2.0 * (double)loss_scale / count);
      OSD_HIP(launch_on_b3t_or_fp32(h, s, g, ea, launch_mse_b3t, launch_mse));
      return OSD_OK;
    }
    // osd_set_loss: the same launch with EpiLoss; rho' of l2 is 2 d, of the other kinds rho' itself
    ea.gscale = (float)((h->loss_kind == OSD_LOSS_L2 ? 2.0 : 1.0) * (double)loss_scale / count);
    EpiLoss::Args el{};
    el.m = ea; el.tw = h->loss_tw_set ? h->loss_tw : nullptr; el.t_index = tc.t_idx; el.kind = h->loss_kind; el.delta = h->loss_delta;
    h->last_train_path |= OSD_TP_LOSS_EPI;
    OSD_HIP(launch_on_b3t_or_fp32(h, s, g, el, launch_loss_b3t, launch_loss));
    return OSD_OK;
  }
  // constraint terms on x0_hat (models/diffusion.py:405) against the batch's x0; their gradient joins dL/d eps_hat
  int constraints() {
    const int D = a.D;
    const int* t_idx = tc.t_idx;
    OSD_HIP(hipMemcpyAsync(h->parts_dev, loss_out, 4, hipMemcpyDeviceToDevice, s));
    const float2* pq = reinterpret_cast<const float2*>(h->d_pq.get());      // x0^ = P x_t + Q out; epsilon keeps its own kernels (their bits)
    if (h->pred_type == OSD_PRED_EPSILON) OSD_HIP(launch_x0hat(s, w.x_t, t_idx, h->d_sqrt_ac, h->d_sqrt_1m, n, D, w.pred));
    else OSD_HIP(launch_row_affine(s, w.x_t, t_idx, pq, w.pred, n, D, w.pred));
    OSD_HIP(hipMemsetAsync(w.cw.acc, 0, (size_t)w.cw.acc_doubles * 8, s));
    OSD_HIP(cons_moments(s, w.pred, D, n, D, w.cw.acc, w.cw.mi_r));
    float* gx = grads ? w.g_x0 : nullptr;
    if (use_pw)
      OSD_HIP(cons_pathway(s, *cp, w.cw, w.pred, D, n, D, (float)h->w_pathway, (float)(h->w_pathway * loss_scale), loss_out, h->parts_dev + 1, gx));
    if (use_me) {
      OSD_HIP(cons_moments(s, x0, D, n, D, w.cw.acc + 2 * (int64_t)D, w.cw.mi_t));
      OSD_HIP(cons_mutexpr(s, *cp, w.cw, w.pred, x0, D, n, D, (float)h->w_mutexpr, (float)(h->w_mutexpr * loss_scale), loss_out, h->parts_dev + 2, gx));
    }
    if (grads && h->pred_type == OSD_PRED_EPSILON) OSD_HIP(launch_x0hat_bwd(s, w.g_x0, t_idx, h->d_sqrt_ac, h->d_sqrt_1m, n, D, w.d_out));
    else if (grads) OSD_HIP(launch_row_affine_bwd(s, w.g_x0, t_idx, pq, n, D, w.d_out));
    return OSD_OK;
  }
  int run(const int32_t* t_index) {
    use_pw = h->cons.n_pathways > 0 && h->w_pathway != 0.0;
    use_me = h->cons.n_a > 0 && h->w_mutexpr != 0.0;
    cp = (use_pw || use_me) && !se_out && !map ? &h->cons : nullptr;      // the row mode and the noise map read the raw output alone
    if (cp && n < 2) { set_error("the constraint losses need at least 2 rows"); return OSD_EINVAL; }
    OSD_TRY(h->parts_dev.reserve(16));
    OSD_TRY(ensure_train_ws(h, s, n, cp, &w));
    h->saved_rows = -1;                    // the workspace no longer matches an osd_denoiser_forward_train call
    squads_bwd = w.sq_gact && squad_backward(h, n, grads != nullptr, events != nullptr);
    OSD_TRY(forward(t_index));
    OSD_TRY(loss());
    if (cp) OSD_TRY(constraints());
    if (!grads) return OSD_OK;
    BackwardPass bp(h, s, w, n, tc.train_mode(), masks, seed, roff, grads, events, squads_bwd);
    bp.dp = h->dp_clip > 0.0 && !se_out;
    OSD_TRY(bp.run(w.x_t, w.xld, tc.t_idx, cond, w.d_out, nullptr, loss_out));
    return tc.finish();
  }
};

}  // namespace osd

using namespace osd;

extern "C" {

int osd_grad_buckets(const osd_config* cfg, int32_t* first, int32_t* last, int max_buckets) {
  if (!cfg) return 0;
  Arch a;
  if (build_arch(*cfg, &a) != OSD_OK) return 0;
  // backward finalises: output_proj, then the blocks last-to-first, then everything before the blocks
  std::vector<std::pair<int, int>> bk;
  bk.push_back({a.pm.out_w, a.pm.out_b});
  for (int b = a.n_blocks - 1; b >= 0; --b) bk.push_back({a.layers[2 * b].w, a.layers[2 * b + 1].beta});
  bk.push_back({0, a.pm.tp_b});
  const int n = (int)bk.size();
  if (first && last)
    for (int i = 0; i < n && i < max_buckets; ++i) { first[i] = bk[i].first; last[i] = bk[i].second; }
  return n;
}

// What a call with gradients under osd_set_dp_clip cannot be: anything in which a row's own gradient is undefined or would reach a leaf
// before its clip factor exists.
static int dp_supported(const osd_handle* h, bool from_src, double loss_scale, void* const* events) {
  const char* why = nullptr;
  if (events || loss_scale != 1.0) why = "data parallel (bucket events, loss_scale != 1) is not supported";
  else if ((h->cons.n_pathways > 0 && h->w_pathway != 0.0) || (h->cons.n_a > 0 && h->w_mutexpr != 0.0))
    why = "the constraint losses are batch statistics: a row has no gradient of its own (osd_set_constraints(h, NULL) clears them)";
  else if (from_src && h->batch_src.idx_b) why = "a mixed-up batch source (idx_b) puts one record into two rows";
  for (const LayerDesc& l : h->arch.layers)
    if (!why && !dgrad_gnbwd_supported(l.gw)) why = "a GroupNorm group width outside the fused GroupNorm backward (32 / 64: hidden widths 256 / 512)";
  if (!why) return OSD_OK;
  set_error("per-row gradient clipping (osd_set_dp_clip): %s", why);
  return OSD_EUNSUPPORTED;
}

// What a call under osd_set_loss_mask cannot be: anything that reads x0 or x0^ outside the masked loss, where a NaN would spread.
static int mask_supported(const osd_handle* h, bool grads) {
  const char* why = nullptr;
  if ((h->cons.n_pathways > 0 && h->w_pathway != 0.0) || (h->cons.n_a > 0 && h->w_mutexpr != 0.0))
    why = "the constraint losses are batch statistics over x0^ and x0, which have no value at an unobserved element (osd_set_constraints(h, NULL) clears them)";
  else if (grads && h->dp_clip > 0.0) why = "per-row gradient clipping (osd_set_dp_clip) is not supported on incomplete rows";
  if (!why) return OSD_OK;
  set_error("masked loss (osd_set_loss_mask): %s", why);
  return OSD_EUNSUPPORTED;
}

// What a call under osd_set_output_link cannot be: anything that would read a logit as x0^.
static int link_supported(const osd_handle* h, bool grads) {
  OSD_TRY(check_output_link(h));
  const char* why = nullptr;
  if ((h->cons.n_pathways > 0 && h->w_pathway != 0.0) || (h->cons.n_a > 0 && h->w_mutexpr != 0.0))
    why = "the constraint losses read the raw output as x0^ (osd_set_constraints(h, NULL) clears them)";
  else if (grads && h->dp_clip > 0.0) why = "per-row gradient clipping (osd_set_dp_clip) is not supported with a linked output";
  if (!why) return OSD_OK;
  set_error("output link (osd_set_output_link): %s", why);
  return OSD_EUNSUPPORTED;
}

// checks in order: ready, rows, (one-shots consumed), null tensors, empty batch, row offset, event count, grads[i], then the device
int osd_train_loss_fwd_bwd(osd_handle* h, const float* x0, const float* cond, int64_t n, const int32_t* t_index, const float* noise,
                           const float* const* masks, uint64_t seed, int64_t row_offset, int flags, float* loss_out,
                           float* const* grads, double loss_scale, void* const* events, int n_events) {
  TrainCall tc{h, n, flags};
  OSD_TRY(tc.begin(true));
  const bool from_src = h->have_batch_src;          // one-shot: consumed (or dropped) by this call
  h->have_batch_src = false;
  const bool cond_drop = h->have_cond_drop;        // one-shot as well (osd_train_condition_dropout)
  h->have_cond_drop = false;
  if ((!from_src && (!x0 || !cond)) || !loss_out) { set_error("null tensor"); return OSD_EINVAL; }
  if (n == 0) { set_error("empty batch"); return OSD_EINVAL; }
  OSD_TRY(check_row_offset(row_offset, n));
  OSD_TRY(tc.check_outputs(events, n_events, grads));
  if (h->loss_mask) OSD_TRY(mask_supported(h, grads != nullptr));      // before any launch: no gradient buffer is touched
  if (h->n_link > 0) OSD_TRY(link_supported(h, grads != nullptr));
  if (grads && h->dp_clip > 0.0) OSD_TRY(dp_supported(h, from_src, loss_scale, events));      // before any launch: no gradient buffer is touched
  OSD_TRY(tc.enter());
  LossStep step{tc, h, h->arch, tc.s, n, x0, cond, noise, masks, seed, (uint32_t)row_offset, loss_out, grads, loss_scale, events, from_src, cond_drop};
  return step.run(t_index);
}

// What osd_row_sq_error and osd_bound_sweep check alike, in order: null handle / tensors, rows, row offset, armed one-shots, precision;
// each then checks its own arguments, and last that the handle is ready.
static int bound_checks(osd_handle* h, const float* x0, const float* cond, int64_t n, int64_t row_offset, const float* se_out) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!x0 || !cond || !se_out) { set_error("null tensor"); return OSD_EINVAL; }
  if (n < 1) { set_error("need at least one row, got %lld", (long long)n); return OSD_EINVAL; }
  OSD_TRY(check_rows(n));
  OSD_TRY(check_row_offset(row_offset, n));
  if (h->have_batch_src || h->have_cond_drop) {
    set_error("a batch source or condition dropout is armed for the next training call; the likelihood calls do not consume it");
    return OSD_ESTATE;
  }
  if (h->precision == 1) { set_error("the per-row squared error runs on the fp32 kernels only (precision 0)"); return OSD_EUNSUPPORTED; }
  if (h->loss_mask) {
    set_error("masked loss (osd_set_loss_mask): the per-row squared error (osd_row_sq_error, osd_bound_sweep) has no masked form; osd_set_loss_mask(h, 0) first");
    return OSD_EUNSUPPORTED;
  }
  if (h->n_link > 0) {
    set_error("output link (osd_set_output_link): the per-row squared error (osd_row_sq_error, osd_bound_sweep) has no Bernoulli form; it is refused, not approximated");
    return OSD_EUNSUPPORTED;
  }
  return OSD_OK;
}

// One launch group of the row mode: n rows, pairs pr.pair0 .. pr.pair0 + n of the grid
static int bound_group(osd_handle* h, hipStream_t s, const float* x0, const float* cond, int64_t n, const PairRows& pr, const int32_t* t_index,
                       const float* noise, uint64_t seed, uint32_t roff, float* se_out) {
  OSD_TRY(h->parts_dev.reserve(16));
  TrainCall tc{h, n, 0};
  tc.s = s;
  LossStep step{tc, h, h->arch, s, n, x0, cond, noise, nullptr, seed, roff, h->parts_dev + 8, nullptr, 1.0, nullptr, false, false};
  step.pairs = &pr; step.se_out = se_out;
  return step.run(t_index);
}

int osd_row_sq_error(osd_handle* h, const float* x0, const float* cond, int64_t n, const int32_t* t_index, const float* noise_in, uint64_t seed,
                     int64_t row_offset, float* se_out) {
  OSD_TRY(bound_checks(h, x0, cond, n, row_offset, se_out));
  if (!t_index) { set_error("t_index is null"); return OSD_EINVAL; }
  OSD_TRY(check_ready(h));
  TrainCall tc{h, n, 0};
  OSD_TRY(tc.enter());
  h->last_train_path = 0;
  // groups of at most bound_rows rows, as the sweep: row r of a group is patient p0 + r
  const int D = h->arch.D, cd = h->arch.cond_dim;
  for (int64_t p0 = 0; p0 < n; p0 += h->bound_rows) {
    const int64_t rows = std::min(h->bound_rows, n - p0);
    const PairRows pr{p0, n, nullptr, nullptr};
    OSD_TRY(bound_group(h, tc.s, x0, cond + p0 * cd, rows, pr, t_index + p0, noise_in ? noise_in + p0 * D : nullptr, seed, (uint32_t)row_offset,
                        se_out + p0));
  }
  return OSD_OK;
}

int osd_bound_sweep(osd_handle* h, const float* x0, const float* cond, int64_t n, const int32_t* timesteps_host, int S, const float* noise_in,
                    uint64_t seed, int64_t row_offset, float* se_out) {
  OSD_TRY(bound_checks(h, x0, cond, n, row_offset, se_out));
  if (S < 1 || !timesteps_host) { set_error("need at least one timestep, got %d", S); return OSD_EINVAL; }
  for (int i = 0; i < S; ++i)
    if (timesteps_host[i] < 0 || timesteps_host[i] >= h->arch.T) {
      set_error("timesteps[%d] = %d is outside [0, %d)", i, (int)timesteps_host[i], h->arch.T);
      return OSD_EINVAL;
    }
  OSD_TRY(check_ready(h));
  TrainCall tc{h, n, 0};
  OSD_TRY(tc.enter());
  hipStream_t s = tc.s;
  h->last_train_path = 0;
  OSD_HIP(hipStreamSynchronize(s));          // an earlier sweep may still read the list
  OSD_TRY(h->bound_ts.reserve(((int64_t)S + 1023) / 1024 * 1024));      // 1024-timestep granules
  OSD_HIP(hipMemcpy(h->bound_ts, timesteps_host, (size_t)S * 4, hipMemcpyHostToDevice));
  // groups of at most bound_rows (timestep, patient) pairs, in pair order: the workspace is bounded whatever n x S is, and a group may
  // end in the middle of a timestep's patients
  const int64_t total = n * (int64_t)S, cap = h->bound_rows;
  const int D = h->arch.D;
  for (int64_t p0 = 0; p0 < total; p0 += cap) {
    const int64_t rows = std::min(cap, total - p0);
    const PairRows pr{p0, n, nullptr, h->bound_ts};
    OSD_TRY(bound_group(h, s, x0, cond, rows, pr, nullptr, noise_in ? noise_in + p0 * D : nullptr, seed, (uint32_t)row_offset, se_out + p0));
  }
  return OSD_OK;
}

// checks in order, all on the host: null handle / tensors, rows, the plan, row offset, armed one-shots, precision, output link, ready
int osd_noise_map(osd_handle* h, const float* x0, const float* cond, int64_t n, const int32_t* timesteps_host, const float* step_coef_host,
                  int32_t n_steps, const float* noise_in, uint64_t seed, int64_t row_offset, float* x_start_out, float* noises_out) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!x0 || !cond || !timesteps_host || !step_coef_host || !x_start_out || (n_steps > 1 && !noises_out)) { set_error("null tensor"); return OSD_EINVAL; }
  if (n < 1) { set_error("need at least one row, got %lld", (long long)n); return OSD_EINVAL; }
  OSD_TRY(check_rows(n));
  const int T = h->arch.T, S = n_steps;
  if (S < 1 || S > T) { set_error("n_steps=%d outside [1,%d]", S, T); return OSD_EINVAL; }
  for (int s = 0; s < S; ++s) {
    if (timesteps_host[s] < 0 || timesteps_host[s] >= T) { set_error("timesteps[%d]=%d outside [0,%d)", s, (int)timesteps_host[s], T); return OSD_EINVAL; }
    if (s > 0 && timesteps_host[s] <= timesteps_host[s - 1]) { set_error("timesteps[%d]=%d does not exceed timesteps[%d]=%d: the plan must strictly increase", s, (int)timesteps_host[s], s - 1, (int)timesteps_host[s - 1]); return OSD_EINVAL; }
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(step_coef_host[4 * s + k])) { set_error("step_coef[%d] is not finite", 4 * s + k); return OSD_EINVAL; }
    const float c = step_coef_host[4 * s + 2];
    if (s == 0 && c != 0.f) { set_error("step_coef[2] = C_0 = %g: the last step draws no z, so C_0 must be 0", (double)c); return OSD_EINVAL; }
    if (s > 0 && !(c > 0.f)) { set_error("step_coef[%d] = C_%d = %g: the noise map solves every step for its draw and needs C_s > 0 (eta > 0)", 4 * s + 2, s, (double)c); return OSD_EINVAL; }
  }
  OSD_TRY(check_row_offset(row_offset, n));
  if (h->have_batch_src || h->have_cond_drop) {
    set_error("a batch source or condition dropout is armed for the next training call; the noise map does not consume it");
    return OSD_ESTATE;
  }
  if (h->precision == 1) { set_error("the noise map runs on the fp32 kernels only (precision 0)"); return OSD_EUNSUPPORTED; }
  if (h->n_link > 0) {
    set_error("output link (osd_set_output_link): a linked model's step is not the plain affine row the noise map inverts; it is refused, not approximated");
    return OSD_EUNSUPPORTED;
  }
  const int D = h->arch.D;
  if (D < 4) { set_error("the noise map keeps a 16-byte record per row in a [rows][D] workspace: D=%d < 4", D); return OSD_EUNSUPPORTED; }
  OSD_TRY(check_ready(h));
  TrainCall tc{h, n, 0};
  OSD_TRY(tc.enter());
  hipStream_t s = tc.s;
  h->last_train_path = 0;
  OSD_HIP(hipStreamSynchronize(s));          // an earlier sweep or map may still read the tables
  OSD_TRY(h->bound_ts.reserve(((int64_t)S + 1023) / 1024 * 1024));      // 1024-level granules, as the sweep
  OSD_TRY(h->map_coef.reserve(((int64_t)S + 1023) / 1024 * 1024 * 4));
  OSD_HIP(hipMemcpy(h->bound_ts, timesteps_host, (size_t)S * 4, hipMemcpyHostToDevice));
  OSD_HIP(hipMemcpy(h->map_coef, step_coef_host, (size_t)S * 16, hipMemcpyHostToDevice));
  if (S == 1) {      // nothing to solve: x_start = y_0
    const MapRows mr{0, n, h->bound_ts, h->map_coef, 1, 0};
    OSD_HIP(launch_q_sample_map(s, x0, cond, h->arch.cond_dim, mr, h->d_sqrt_ac, h->d_sqrt_1m, noise_in, n, D, seed, (uint32_t)row_offset, nullptr, 0,
                                nullptr, nullptr, x_start_out, nullptr, nullptr, nullptr));
    return OSD_OK;
  }
  // groups of at most bound_rows (level, patient) pairs over the levels 1 .. S-1, in pair order, as the sweep; level 0 draws nothing and
  // does not run: y_0 is formed by level 1's rows
  const int64_t total = n * (int64_t)(S - 1), cap = h->bound_rows;
  OSD_TRY(h->parts_dev.reserve(16));
  for (int64_t p0 = 0; p0 < total; p0 += cap) {
    const int64_t rows = std::min(cap, total - p0);
    const MapRows mr{p0, n, h->bound_ts, h->map_coef, S, 1};
    TrainCall gc{h, rows, 0};
    gc.s = s;
    LossStep step{gc, h, h->arch, s, rows, x0, cond, noise_in, nullptr, seed, (uint32_t)row_offset, h->parts_dev + 8, nullptr, 1.0, nullptr, false, false};
    step.map = &mr; step.z_out = noises_out; step.x_start = x_start_out;
    OSD_TRY(step.run(nullptr));
  }
  return OSD_OK;
}

int osd_train_batch_source(osd_handle* h, const float* data, int64_t ld_data, const float* cond, int64_t ld_cond, const int64_t* idx_a,
                           const int64_t* idx_b, double lam) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!data || !cond) { set_error("null dataset tensor"); return OSD_EINVAL; }
  if (ld_data < h->arch.D || ld_cond < h->arch.cond_dim) { set_error("dataset row strides %lld / %lld are smaller than the model's dims", (long long)ld_data, (long long)ld_cond); return OSD_EINVAL; }
  if (!(lam >= 0.0 && lam <= 1.0)) { set_error("lam must be in [0,1]"); return OSD_EINVAL; }
  BatchSrc b{};
  b.data = data; b.ldd = ld_data; b.cond = cond; b.ldc = ld_cond; b.idx_a = idx_a; b.idx_b = idx_b;
  // python: lam and (1 - lam) are float64 scalars; torch multiplies an fp32 tensor by each as fp32 (launch_mixup)
  b.lam = (float)lam; b.oml = (float)(1.0 - lam);
  h->batch_src = b;
  h->have_batch_src = true;
  return OSD_OK;
}

int osd_train_condition_dropout(osd_handle* h, const float* null_cond_host, double p, const float* keep_dev) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!(p >= 0.0 && p <= 1.0)) { set_error("condition dropout p must be in [0,1]"); return OSD_EINVAL; }
  h->have_cond_drop = false;
  if (p == 0.0 && !keep_dev) return OSD_OK;          // nothing to drop: the next training call is the plain one
  if (!null_cond_host) { set_error("null_cond is null"); return OSD_EINVAL; }
  for (int i = 0; i < h->arch.cond_dim; ++i)
    if (!std::isfinite(null_cond_host[i])) { set_error("null_cond[%d] is not finite", i); return OSD_EINVAL; }
  const float* dev = nullptr;
  OSD_TRY(upload_null_cond(h, 1, null_cond_host, &dev));
  h->cond_drop_p = (float)p; h->cond_drop_keep = keep_dev;
  h->have_cond_drop = true;
  return OSD_OK;
}

// checks in order: ready, rows, null tensors / empty batch, row offset, then the device
int osd_denoiser_forward_train(osd_handle* h, const float* x_t, const int32_t* t_index, const float* cond, int64_t n,
                               const float* const* masks, uint64_t seed, int64_t row_offset, int flags, float* eps_out) {
  TrainCall tc{h, n, flags};
  OSD_TRY(tc.begin(false));
  if (!x_t || !t_index || !cond || !eps_out || n == 0) { set_error("null tensor or empty batch"); return OSD_EINVAL; }
  OSD_TRY(check_row_offset(row_offset, n));
  const Arch& a = h->arch;
  OSD_TRY(tc.enter());
  hipStream_t s = tc.s;
  TrainWs w;
  OSD_TRY(ensure_train_ws(h, s, n, nullptr, &w));
  h->saved_rows = -1;
  OSD_TRY(tc.timesteps(t_index));
  OSD_TRY(refresh_derived(h, s));
  OSD_TRY(cond_embed_fwd(h, s, cond, n, w));
  TrunkIn in{};
  in.x = x_t; in.ldx = a.D; in.n = n; in.t_index = tc.t_idx; in.train = tc.train_mode(); in.save = true;
  in.masks = masks; in.seed = seed; in.row_offset = (uint32_t)row_offset; in.drop_step = 0;
  OSD_TRY(run_trunk(h, s, w.f, in));
  GemmArgs g = output_proj_args(h, w.f, n);
  OSD_HIP(launch_linear(s, g, true, true, h->params[a.pm.out_b], eps_out, a.D, false, false));
  h->saved_rows = n;
  return tc.finish();
}

// checks in order: ready, rows, null tensors / empty batch, saved activations, event count, grads[i], row offset, then the device
int osd_denoiser_backward(osd_handle* h, const float* x_t, const int32_t* t_index, const float* cond, int64_t n, const float* dout,
                          const float* const* masks, uint64_t seed, int64_t row_offset, int flags, float* const* grads, float* dx_t,
                          void* const* events, int n_events) {
  TrainCall tc{h, n, flags};
  OSD_TRY(tc.begin(true));
  if (!x_t || !t_index || !cond || !dout || !grads || n == 0) { set_error("null tensor or empty batch"); return OSD_EINVAL; }
  // an upstream gradient of the caller's own loss: whether its rows are per-patient terms is not this call's to know, so it never clips --
  // and never hands back unclipped gradients while a per-row bound is set
  if (h->dp_clip > 0.0) { set_error("per-row gradient clipping (osd_set_dp_clip) covers osd_train_loss_fwd_bwd only"); return OSD_EUNSUPPORTED; }
  if (h->saved_rows != n) { set_error("osd_denoiser_backward needs the activations of an osd_denoiser_forward_train call on the same %lld rows", (long long)n); return OSD_ESTATE; }
  OSD_TRY(tc.check_outputs(events, n_events, grads));
  OSD_TRY(check_row_offset(row_offset, n));
  OSD_TRY(tc.enter());
  const Arch& a = h->arch;
  TrainWs w;
  carve_train(a, h->train_arena, n, nullptr, &w);       // same carving as the forward call: pointers to its activations
  OSD_TRY(tc.timesteps(t_index));
  ZeroList zl{};
  add_backward_zeros(a, w, grads, &zl);
  OSD_HIP(launch_zero_many(tc.s, zl));
  // per-layer dgrads: the forward call packed no transposed weights and there is no loss word for the squads to poison
  BackwardPass bp(h, tc.s, w, n, tc.train_mode(), masks, seed, (uint32_t)row_offset, grads, events, false);
  OSD_TRY(bp.run(x_t, a.D, tc.t_idx, cond, dout, dx_t, nullptr));
  return tc.finish();
}

int osd_set_constraints(osd_handle* h, const osd_constraints* c) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  if (h->stream) OSD_HIP(hipStreamSynchronize(h->stream));
  ConsPlan fresh;
  if (c) {
    if (c->pathway_weight < 0 || c->mutexpr_weight < 0) { set_error("constraint weights must be >= 0"); return OSD_EINVAL; }
    OSD_TRY(cons_build_plan(c->pathway_offsets, c->pathway_members, c->n_pathways, c->cols_a, c->n_a, c->cols_b, c->n_b, h->arch.D, &fresh));
  }
  h->cons = std::move(fresh);      // the old plan goes with `fresh`
  h->w_pathway = c ? c->pathway_weight : 0.0;
  h->w_mutexpr = c ? c->mutexpr_weight : 0.0;
  return OSD_OK;
}

int osd_set_loss(osd_handle* h, int kind, double huber_delta, const float* t_weights_host) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (kind != OSD_LOSS_L2 && kind != OSD_LOSS_L1 && kind != OSD_LOSS_HUBER) { set_error("unknown loss kind %d (OSD_LOSS_L2, OSD_LOSS_L1 or OSD_LOSS_HUBER)", kind); return OSD_EINVAL; }
  if (!(huber_delta > 0.0) || !std::isfinite(huber_delta) || !((float)huber_delta > 0.f) || !std::isfinite((float)huber_delta)) {
    set_error("huber_delta must be positive and finite, got %g", huber_delta);
    return OSD_EINVAL;
  }
  const int T = h->arch.T;
  if (t_weights_host)
    for (int i = 0; i < T; ++i)
      if (!std::isfinite(t_weights_host[i]) || t_weights_host[i] < 0.f) { set_error("loss weight [%d] = %g is negative or not finite", i, (double)t_weights_host[i]); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  if (h->stream) OSD_HIP(hipStreamSynchronize(h->stream));       // a training call in flight may still read the table
  if (t_weights_host) {
    OSD_TRY(h->loss_tw.reserve(T));
    OSD_HIP(hipMemcpy(h->loss_tw, t_weights_host, (size_t)T * sizeof(float), hipMemcpyHostToDevice));
  }
  h->loss_tw_set = t_weights_host != nullptr;
  h->loss_kind = kind;
  h->loss_delta = (float)huber_delta;
  return OSD_OK;
}

int osd_set_loss_mask(osd_handle* h, int enable) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  h->loss_mask = enable != 0;      // host state alone: read when the next call is issued
  return OSD_OK;
}

int osd_get_loss_parts(osd_handle* h, float* parts_host3) {
  if (!h || !parts_host3) { set_error("null argument"); return OSD_EINVAL; }
  if (!h->parts_dev || !(h->cons.n_pathways > 0 || h->cons.n_a > 0)) { set_error("no constraint losses are configured on this handle"); return OSD_ESTATE; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_HIP(hipMemcpyAsync(parts_host3, h->parts_dev, 12, hipMemcpyDeviceToHost, h->stream));
  OSD_HIP(hipStreamSynchronize(h->stream));
  return OSD_OK;
}

// The hyper-parameters of one fused clip_grad_norm_ + AdamW step, as the four entry points receive them.
struct AdamHyper { double lr, beta1, beta2, eps, weight_decay, max_norm; int64_t step; };
// the DP-SGD variants: Gaussian noise of this standard deviation on every gradient element instead of the batch clip (max_norm is then 0)
struct DpNoise { double std; uint64_t seed; };

// The checked body of the four AdamW entry points.  `h`: the handle-taking variants, whose stream, device and norm workspace are
// the handle's; null for the stream-taking ones, which bring their own.  `want_ema`: the EMA variants, which reject a null ema and
// a decay outside [0, 1] before any device call.
static int clip_adamw_step(osd_handle* h, hipStream_t stream, int device, double* norm_ws, float* param, float* grad, float* exp_avg,
                           float* exp_avg_sq, int64_t numel, const AdamHyper& hp, float* grad_norm_out, bool want_ema, float* ema, double ema_decay,
                           const DpNoise* dp = nullptr) {
  if ((!h && !norm_ws && !dp) || !param || !grad || !exp_avg || !exp_avg_sq) { set_error("null argument"); return OSD_EINVAL; }
  if (want_ema && !ema) { set_error("null argument"); return OSD_EINVAL; }
  if (want_ema && !(ema_decay >= 0.0 && ema_decay <= 1.0)) { set_error("ema_decay must be in [0, 1]"); return OSD_EINVAL; }
  if (numel <= 0 || hp.step < 1) { set_error("numel and step must be positive"); return OSD_EINVAL; }
  if (dp && (!(dp->std >= 0.0) || !std::isfinite(dp->std) || !std::isfinite((float)dp->std))) { set_error("noise_std must be finite and >= 0, got %g", dp->std); return OSD_EINVAL; }
  if (dp && hp.step > 0xffffffffll) { set_error("step does not fit the 32-bit Philox counter"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h ? h->cfg.device : device));
  if (h) {
    if (!dp) OSD_TRY(h->normsq_dev.reserve(256));
    // the handle's own optimizer is about to change parameters it may hold derived copies of (t_emb table, packed input_proj /
    // output_proj, chain and bf16x3 weight copies): the next forward / sampling entry point refreshes them (api.hip: ensure_packed)
    h->w_packed_stale = true;
    stream = h->stream; norm_ws = h->normsq_dev;
  }
  AdamArgs a{};
  const double bc1 = 1.0 - pow(hp.beta1, (double)hp.step);
  const double bc2 = 1.0 - pow(hp.beta2, (double)hp.step);
  a.decay = (float)(1.0 - hp.lr * hp.weight_decay);
  a.one_minus_b1 = (float)(1.0 - hp.beta1);
  a.b2 = (float)hp.beta2;
  a.one_minus_b2 = (float)(1.0 - hp.beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)hp.eps;
  a.neg_step_size = (float)(-(hp.lr / bc1));
  a.max_norm = (float)hp.max_norm;
  if (dp) {
    OSD_HIP(launch_dp_adamw(stream, param, grad, exp_avg, exp_avg_sq, numel, a, (float)dp->std, dp->seed, (uint32_t)hp.step, ema, (float)(1.0 - ema_decay)));
    return OSD_OK;
  }
  OSD_HIP(launch_clip_adamw(stream, param, grad, exp_avg, exp_avg_sq, numel, a, norm_ws, grad_norm_out, ema, (float)(1.0 - ema_decay)));
  return OSD_OK;
}

int osd_clip_adamw_step(osd_handle* h, float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, double lr,
                        double beta1, double beta2, double eps, double weight_decay, double max_norm, int64_t step, float* grad_norm_out) {
  if (!h) { set_error("null argument"); return OSD_EINVAL; }
  return clip_adamw_step(h, nullptr, 0, nullptr, param, grad, exp_avg, exp_avg_sq, numel, {lr, beta1, beta2, eps, weight_decay, max_norm, step},
                         grad_norm_out, false, nullptr, 0.0);
}

int osd_nn_clip_adamw_step(void* stream, int device, double* normsq_ws, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                           int64_t numel, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                           int64_t step, float* grad_norm_out) {
  return clip_adamw_step(nullptr, (hipStream_t)stream, device, normsq_ws, param, grad, exp_avg, exp_avg_sq, numel,
                         {lr, beta1, beta2, eps, weight_decay, max_norm, step}, grad_norm_out, false, nullptr, 0.0);
}

int osd_clip_adamw_ema_step(osd_handle* h, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, double lr,
                            double beta1, double beta2, double eps, double weight_decay, double max_norm, int64_t step, double ema_decay,
                            float* grad_norm_out) {
  if (!h) { set_error("null argument"); return OSD_EINVAL; }
  return clip_adamw_step(h, nullptr, 0, nullptr, param, grad, exp_avg, exp_avg_sq, numel, {lr, beta1, beta2, eps, weight_decay, max_norm, step},
                         grad_norm_out, true, ema, ema_decay);
}

int osd_nn_clip_adamw_ema_step(void* stream, int device, double* normsq_ws, float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                               float* ema, int64_t numel, double lr, double beta1, double beta2, double eps, double weight_decay,
                               double max_norm, int64_t step, double ema_decay, float* grad_norm_out) {
  return clip_adamw_step(nullptr, (hipStream_t)stream, device, normsq_ws, param, grad, exp_avg, exp_avg_sq, numel,
                         {lr, beta1, beta2, eps, weight_decay, max_norm, step}, grad_norm_out, true, ema, ema_decay);
}

// The checked body of the two grouped entry points (osdiff.h): everything below the last set_error() is the first device call.
static int group_adamw_step(osd_handle* h, hipStream_t stream, int device, double* norm_ws, float* param, float* grad, float* exp_avg,
                            float* exp_avg_sq, float* ema, const float* anchor, int64_t numel, const osd_param_group* groups, int n_groups,
                            const AdamHyper& hp, double ema_decay, float* grad_norm_out) {
  static_assert(OSD_MAX_PARAM_GROUPS == GROUPS_MAX && OSD_GROUP_WS_DOUBLES == GROUP_WS_DOUBLES, "osdiff.h and kernels_train.h disagree");
  if ((!h && !norm_ws) || !param || !grad || !exp_avg || !exp_avg_sq || !groups) { set_error("null argument"); return OSD_EINVAL; }
  if (ema && !(ema_decay >= 0.0 && ema_decay <= 1.0)) { set_error("ema_decay must be in [0, 1]"); return OSD_EINVAL; }
  if (numel <= 0 || hp.step < 1) { set_error("numel and step must be positive"); return OSD_EINVAL; }
  if (n_groups < 1 || n_groups > OSD_MAX_PARAM_GROUPS) { set_error("n_groups=%d outside [1, %d]", n_groups, OSD_MAX_PARAM_GROUPS); return OSD_EINVAL; }
  const double bc1 = 1.0 - pow(hp.beta1, (double)hp.step);
  const double bc2 = 1.0 - pow(hp.beta2, (double)hp.step);
  std::vector<int64_t> ends((size_t)n_groups);
  std::vector<GroupConst> consts((size_t)n_groups);
  int64_t at = 0;
  for (int k = 0; k < n_groups; ++k) {
    const osd_param_group& gr = groups[k];
    if (gr.begin != at || gr.end <= gr.begin || gr.end > numel) {
      set_error("group %d is [%lld, %lld): the groups must be sorted, non-empty, non-overlapping and cover [0, %lld) (expected begin %lld)", k,
                (long long)gr.begin, (long long)gr.end, (long long)numel, (long long)at);
      return OSD_EINVAL;
    }
    at = gr.end;
    const float sc[3] = {gr.lr_scale, gr.wd_scale, gr.l2sp};
    for (float x : sc)
      if (!(x >= 0.f) || !std::isfinite(x)) { set_error("group %d: lr_scale, wd_scale and l2sp must be finite and >= 0, got %g", k, (double)x); return OSD_EINVAL; }
    if (gr.l2sp > 0.f && !anchor) { set_error("group %d has l2sp=%g but anchor is null", k, (double)gr.l2sp); return OSD_EINVAL; }
    const double lr_k = hp.lr * (double)gr.lr_scale;
    ends[(size_t)k] = gr.end;
    consts[(size_t)k] = {(float)(1.0 - lr_k * hp.weight_decay * (double)gr.wd_scale), (float)(-(lr_k / bc1)), (float)(lr_k * (double)gr.l2sp),
                         gr.lr_scale != 0.f ? 1 : 0};      // frozen iff lr_scale == 0
  }
  if (at != numel) { set_error("the groups end at %lld, not at numel=%lld", (long long)at, (long long)numel); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h ? h->cfg.device : device));
  if (h) {
    OSD_TRY(h->normsq_dev.reserve(OSD_GROUP_WS_DOUBLES, h->stream));
    h->w_packed_stale = true;      // as osd_clip_adamw_step: the next forward / sampling entry point refreshes the derived weight copies
    stream = h->stream; norm_ws = h->normsq_dev;
  }
  AdamArgs a{};
  a.one_minus_b1 = (float)(1.0 - hp.beta1);
  a.b2 = (float)hp.beta2;
  a.one_minus_b2 = (float)(1.0 - hp.beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)hp.eps;
  a.max_norm = (float)hp.max_norm;
  OSD_HIP(launch_group_adamw(stream, param, grad, exp_avg, exp_avg_sq, ema, (float)(1.0 - ema_decay), anchor, numel, a, ends.data(), consts.data(),
                             n_groups, norm_ws, grad_norm_out));
  return OSD_OK;
}

int osd_group_adamw_step(osd_handle* h, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, const float* anchor, int64_t numel,
                         const osd_param_group* groups_host, int n_groups, double lr, double beta1, double beta2, double eps, double weight_decay,
                         double max_norm, int64_t step, double ema_decay, float* grad_norm_out) {
  if (!h) { set_error("null argument"); return OSD_EINVAL; }
  return group_adamw_step(h, nullptr, 0, nullptr, param, grad, exp_avg, exp_avg_sq, ema, anchor, numel, groups_host, n_groups,
                          {lr, beta1, beta2, eps, weight_decay, max_norm, step}, ema_decay, grad_norm_out);
}

int osd_nn_group_adamw_step(void* stream, int device, double* normsq_ws, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                            const float* anchor, int64_t numel, const osd_param_group* groups_host, int n_groups, double lr, double beta1,
                            double beta2, double eps, double weight_decay, double max_norm, int64_t step, double ema_decay, float* grad_norm_out) {
  return group_adamw_step(nullptr, (hipStream_t)stream, device, normsq_ws, param, grad, exp_avg, exp_avg_sq, ema, anchor, numel, groups_host,
                          n_groups, {lr, beta1, beta2, eps, weight_decay, max_norm, step}, ema_decay, grad_norm_out);
}

int osd_dp_adamw_step(osd_handle* h, float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, double lr, double beta1,
                      double beta2, double eps, double weight_decay, double noise_std, uint64_t seed, int64_t step) {
  if (!h) { set_error("null argument"); return OSD_EINVAL; }
  const DpNoise dp{noise_std, seed};
  return clip_adamw_step(h, nullptr, 0, nullptr, param, grad, exp_avg, exp_avg_sq, numel, {lr, beta1, beta2, eps, weight_decay, 0.0, step}, nullptr,
                         false, nullptr, 0.0, &dp);
}

int osd_nn_dp_adamw_step(void* stream, int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t numel, double lr,
                         double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed, int64_t step) {
  const DpNoise dp{noise_std, seed};
  return clip_adamw_step(nullptr, (hipStream_t)stream, device, nullptr, param, grad, exp_avg, exp_avg_sq, numel,
                         {lr, beta1, beta2, eps, weight_decay, 0.0, step}, nullptr, false, nullptr, 0.0, &dp);
}

int osd_dp_adamw_ema_step(osd_handle* h, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, double lr,
                          double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed, int64_t step,
                          double ema_decay) {
  if (!h) { set_error("null argument"); return OSD_EINVAL; }
  const DpNoise dp{noise_std, seed};
  return clip_adamw_step(h, nullptr, 0, nullptr, param, grad, exp_avg, exp_avg_sq, numel, {lr, beta1, beta2, eps, weight_decay, 0.0, step}, nullptr,
                         true, ema, ema_decay, &dp);
}

int osd_nn_dp_adamw_ema_step(void* stream, int device, float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel,
                             double lr, double beta1, double beta2, double eps, double weight_decay, double noise_std, uint64_t seed,
                             int64_t step, double ema_decay) {
  const DpNoise dp{noise_std, seed};
  return clip_adamw_step(nullptr, (hipStream_t)stream, device, nullptr, param, grad, exp_avg, exp_avg_sq, numel,
                         {lr, beta1, beta2, eps, weight_decay, 0.0, step}, nullptr, true, ema, ema_decay, &dp);
}

}  // extern "C"
