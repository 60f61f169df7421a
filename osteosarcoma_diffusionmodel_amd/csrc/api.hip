// api.hip -- C ABI of libosdiff.so (include/osdiff.h): handle management, the denoiser
// forward pass (forward_request), q_sample / p_sample / the reverse chain.  sample_request
// validates an osd_sample_chain* call into a ChainJob (handle.h), sample_plan picks the engine
// and chain_chunk drives the per-layer kernels (eager or hipGraph-replayed).
// Training entry points live in train.hip.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <new>
#include "handle.h"
#include "kernels.h"
#include "fwd.h"
#include "launch.h"
#include "split.h"
#include "dp.h"

namespace osd {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

std::vector<KernelReg>& kernel_registry() {
  static std::vector<KernelReg> r;
  return r;
}
hipError_t prepare_kernels() {
  for (const KernelReg& k : kernel_registry()) {
    hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds_bytes);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

int build_arch(const osd_config& c, Arch* a) {
  if (c.mutation_dim < 0 || c.expression_dim < 0 || c.pathway_dim < 0 || c.condition_dim <= 0) { set_error("bad feature dims"); return OSD_EINVAL; }
  a->D = c.mutation_dim + c.expression_dim + c.pathway_dim;
  if (a->D <= 0) { set_error("data_dim must be positive"); return OSD_EINVAL; }
  if (c.n_hidden < 1 || c.n_hidden > OSD_MAX_HIDDEN) { set_error("n_hidden must be in [1,%d]", OSD_MAX_HIDDEN); return OSD_EINVAL; }
  if (c.num_steps < 1) { set_error("num_steps must be >= 1"); return OSD_EINVAL; }
  if (c.time_dim < 4 || (c.time_dim & 1)) { set_error("time_dim (latent_dim) must be even and >= 4"); return OSD_EINVAL; }
  // models/diffusion.py:285 hard-wires the condition embedding width to 64 while cond_proj
  // expects latent_dim // 2 inputs (:292): only latent_dim 128/129 constructs a working model.
  if (c.time_dim / 2 != 64) { set_error("latent_dim // 2 must equal 64 (reference ConditionalEmbedding width)"); return OSD_EINVAL; }
  if (!(c.dropout_p >= 0.f && c.dropout_p < 1.f)) { set_error("dropout must be in [0,1)"); return OSD_EINVAL; }
  a->cond_dim = c.condition_dim;
  a->time_dim = c.time_dim;
  a->cond_width = 64;
  a->T = c.num_steps;
  a->hidden.assign(c.hidden_dims, c.hidden_dims + c.n_hidden);
  for (int hdim : a->hidden) {
    if (hdim <= 0 || hdim % 8) { set_error("hidden dims must be positive multiples of 8 (GroupNorm(8, C))"); return OSD_EINVAL; }
    if (!gn_width_supported(hdim / 8)) { set_error("hidden dim %d: group width %d is outside the fused kernels (power of two in [4,128])", hdim, hdim / 8); return OSD_EUNSUPPORTED; }
  }
  const int L = c.n_hidden;
  a->H0 = a->hidden[0];
  a->n_enc = L - 1;
  a->n_blocks = 2 * (L - 1) + 1;
  a->layers.clear();
  a->block_out.clear();
  ParamMap& pm = a->pm;
  pm.numel.clear();
  int idx = 0;
  auto P = [&](int64_t n) { pm.numel.push_back(n); return idx++; };
  pm.ce0_w = P((int64_t)64 * c.condition_dim); pm.ce0_b = P(64);
  pm.ce2_w = P(64 * 64); pm.ce2_b = P(64);
  pm.in_w = P((int64_t)a->H0 * a->D); pm.in_b = P(a->H0);
  pm.cp_w = P((int64_t)a->H0 * (c.time_dim / 2)); pm.cp_b = P(a->H0);
  pm.tp_w = P((int64_t)a->H0 * c.time_dim); pm.tp_b = P(a->H0);
  int bi = 0;
  auto block = [&](int k1, int k2, int n) {
    LayerDesc l1{k1, k2, n, 0, 0, 0, 0, n / 8, bi, 0};
    l1.w = P((int64_t)n * (k1 + k2)); l1.b = P(n); l1.gamma = P(n); l1.beta = P(n);
    LayerDesc l2{n, 0, n, 0, 0, 0, 0, n / 8, bi, 1};
    l2.w = P((int64_t)n * n); l2.b = P(n); l2.gamma = P(n); l2.beta = P(n);
    a->layers.push_back(l1); a->layers.push_back(l2);
    a->block_out.push_back(n);
    ++bi;
  };
  int cin = a->hidden[0];
  for (int i = 1; i < L; ++i) { block(cin, 0, a->hidden[i]); cin = a->hidden[i]; }
  block(cin, 0, cin);
  int cur = a->hidden[L - 1];
  for (int i = L - 2; i >= 0; --i) { block(cur, a->hidden[i + 1], a->hidden[i]); cur = a->hidden[i]; }
  pm.out_w = P((int64_t)a->D * cur); pm.out_b = P(a->D);
  pm.n_params = idx;
  int64_t per = 64 + 64 + 2 * (int64_t)a->H0;
  for (int n : a->block_out) per += 2 * (int64_t)n;
  a->act_floats_per_row = per;
  return OSD_OK;
}

int device_alloc(void** p, size_t bytes) {
  if (hipMalloc(p, bytes) == hipSuccess) return OSD_OK;
  (void)hipGetLastError();
  *p = nullptr;
  set_error("hipMalloc of %lld bytes failed", (long long)bytes);
  return OSD_ENOMEM;
}

// Carve forward activations for n rows out of `base`; returns floats used.
int64_t carve_fwd(const Arch& a, float* base, int64_t n, bool train, FwdWs* ws) {
  int64_t off = 0;
  auto take = [&](int64_t floats) { float* p = base ? base + off : nullptr; off += up64(floats); return p; };
  ws->ce1 = take(n * 64); ws->ce2 = take(n * 64);
  ws->cproj = take(n * a.H0); ws->h0 = take(n * a.H0);
  ws->mid.resize(a.n_blocks); ws->out.resize(a.n_blocks);
  ws->z1.assign(a.n_blocks, nullptr); ws->z2.assign(a.n_blocks, nullptr);
  ws->st1.assign(a.n_blocks, nullptr); ws->st2.assign(a.n_blocks, nullptr);
  for (int b = 0; b < a.n_blocks; ++b) {
    const int64_t c = a.block_out[b];
    ws->mid[b] = take(n * c); ws->out[b] = take(n * c);
    if (train) {
      ws->z1[b] = take(n * c); ws->z2[b] = take(n * c);
      ws->st1[b] = take(n * 16); ws->st2[b] = take(n * 16);
    }
  }
  return off;
}

// ConditionalEmbedding + cond_proj (models/diffusion.py:101-105, 226): cproj[n][H0]
int run_cond(osd_handle* h, hipStream_t s, const float* cond, int64_t n, const FwdWs& ws) {
  const Arch& a = h->arch;
  const ParamMap& pm = a.pm;
  GemmArgs g{};
  g.A = h->params[pm.ce0_w]; g.lda = a.cond_dim; g.B0 = cond; g.ldb0 = a.cond_dim; g.K0 = a.cond_dim;
  g.F = 64; g.P = (int)n; g.K = a.cond_dim;
  OSD_HIP(launch_linear(s, g, true, true, h->params[pm.ce0_b], ws.ce1, 64, true, false));
  g.A = h->params[pm.ce2_w]; g.lda = 64; g.B0 = ws.ce1; g.ldb0 = 64; g.K0 = 64; g.K = 64;
  OSD_HIP(launch_linear(s, g, true, true, h->params[pm.ce2_b], ws.ce2, 64, false, false));
  g.A = h->params[pm.cp_w]; g.lda = 64; g.B0 = ws.ce2; g.ldb0 = 64; g.K0 = 64; g.K = 64; g.F = a.H0;
  OSD_HIP(launch_linear(s, g, true, true, h->params[pm.cp_b], ws.cproj, a.H0, false, false));
  return OSD_OK;
}

static int prof_mark(osd_handle* h, hipStream_t s) {
  if (h->prof_events) {
    if (h->prof_i >= (int)h->prof_events->size()) { set_error("profile event overflow"); return OSD_EINVAL; }
    OSD_HIP(hipEventRecord((*h->prof_events)[h->prof_i++], s));
  }
  return OSD_OK;
}

static hipError_t launch_in(hipStream_t s, const GemmArgs& g, const EpiInput::Args& ea) { return launch_input(s, g, ea, true); }
static hipError_t launch_in(hipStream_t s, const GemmArgs& g, const EpiInputGuided::Args& ea) { return launch_input_guided(s, g, ea, true); }
static hipError_t launch_in_splitk(hipStream_t s, const GemmArgs& g, const EpiInput::Args& ea, float* slabs, int slices) {
  return launch_input_splitk(s, g, ea, slabs, slices);
}
static hipError_t launch_in_splitk(hipStream_t s, const GemmArgs& g, const EpiInputGuided::Args& ea, float* slabs, int slices) {
  return launch_input_guided_splitk(s, g, ea, slabs, slices);
}

// input_proj with either epilogue (EpiInput / EpiInputGuided): K in slices over workgroups where the caller provides slabs and the
// shape allows (k_fused.hip), else one pass
template <class EpiArgs>
static int run_input_proj(osd_handle* h, hipStream_t s, const TrunkIn& in, GemmArgs g, const EpiArgs& ea) {
  const Arch& a = h->arch;
  if (in.in_slices > 1 && in.in_slabs) {
    const hipError_t e = launch_in_splitk(s, g, ea, in.in_slabs, in.in_slices);
    if (e == hipSuccess) return prof_mark(h, s);
    if (e != hipErrorInvalidValue) OSD_HIP(e);
    (void)hipGetLastError();
  }
  hipError_t e = launch_in(s, g, ea);
  if (e == hipErrorInvalidValue && g.a_kmax > 0) {
    // the clamped-weight path needs 16-byte aligned parameter pointers (launch.h: glds_ok / fast_ok), which the caller of
    // osd_load_weights does not owe us: pack the padded copy after all and read that (x already has zero pad columns)
    (void)hipGetLastError();
    OSD_HIP(launch_copy2d(s, h->params[a.pm.in_w], a.D, h->w_in_packed, h->w_in_ld, a.H0, a.D));
    g.A = h->w_in_packed; g.lda = h->w_in_ld; g.a_kmax = 0;
    e = launch_in(s, g, ea);
    if (in.path) *in.path |= OSD_TP_INPUT_REPACK;
  }
  OSD_HIP(e);
  return prof_mark(h, s);
}

// input_proj + blocks (models/diffusion.py:229-251); result in ws.out[n_blocks-1].
int run_trunk(osd_handle* h, hipStream_t s, const FwdWs& ws, const TrunkIn& in) {
  const Arch& a = h->arch;
  const ParamMap& pm = a.pm;
  const int n = (int)in.n;
  const bool guided = in.guide_m > 0;      // one input_proj GEMM over the state rows, both branches' h0 from its epilogue (or the split-K reduce)
  {
    GemmArgs g{};
    const int kx = in.kx > 0 ? in.kx : a.D;
    g.A = h->w_in_packed; g.lda = h->w_in_ld; g.B0 = in.x; g.ldb0 = in.ldx; g.K0 = kx;
    g.F = a.H0; g.P = guided ? (int)in.guide_m : n; g.K = kx;
    if (in.a_unpacked && !guided) { g.A = h->params[pm.in_w]; g.lda = a.D; g.a_kmax = a.D; }
    g.ksplit = in.ksplit ? 1 : 0;
    const EpiInput::Args ea{h->params[pm.in_b], in.temb ? in.temb : h->d_temb, a.H0, in.t_index, in.t_dev, in.t_imm, ws.cproj, a.H0, ws.h0, a.H0};
    if (guided) {
      OSD_TRY(run_input_proj(h, s, in, g, EpiInputGuided::Args{ea.bias, ea.temb, ea.ldt, ea.t_index, ea.t_dev, ea.t_imm, ea.cproj, ea.ldc, in.cproj0,
                                                              ea.out, ea.ldo, (long long)in.guide_m * a.H0}));
    } else {
      OSD_TRY(run_input_proj(h, s, in, g, ea));
    }
  }
  if (in.input_only) return OSD_OK;
  const bool drop = in.train && h->cfg.dropout_p > 0.f;
  // one Linear + GroupNorm + SiLU launch: the first half of a block (dropout behind it, the decoder's skip input beside x) or the second
  auto layer = [&](const LayerDesc& l, const float* x, float* out, float* z, float* stats) -> int {
    const int b = l.block;
    GemmArgs g{};
    g.A = h->params[l.w]; g.lda = l.K1 + l.K2; g.B0 = x; g.ldb0 = l.K1; g.K0 = l.K1;
    if (l.K2 > 0) { g.B1 = ws.out[a.skip_of(b)]; g.ldb1 = a.block_out[a.skip_of(b)]; }
    g.F = l.N; g.P = n; g.K = l.K1 + l.K2; g.ksplit = in.ksplit ? 1 : 0;
    GnArgs ga{};
    ga.bias = h->params[l.b]; ga.gamma = h->params[l.gamma]; ga.beta = h->params[l.beta];
    ga.out = out; ga.ldo = l.N;
    ga.z_out = in.save ? z : nullptr; ga.ldz = l.N; ga.stats = in.save ? stats : nullptr;
    if (drop && l.half == 0) {
      ga.drop_mode = in.masks ? 1 : 2;
      ga.mask = in.masks ? in.masks[b] : nullptr; ga.ldm = l.N;
      ga.keep_scale = (float)(1.0 / (1.0 - (double)h->cfg.dropout_p)); ga.p_drop = h->cfg.dropout_p;
      ga.seed = in.seed; ga.row_offset = in.row_offset; ga.step = in.drop_step; ga.tag = TAG_DROPOUT + (uint32_t)b;
      ga.step_dev = in.drop_step_dev;
      OSD_HIP(launch_gn_silu_drop(s, g, l.gw, ga));
      return prof_mark(h, s);
    }
    // small batches: a deep layer is a few dozen tiles of 16-32 sequential K steps -- K in slices over workgroups + a reduce kernel
    if (in.gn_slices >= 2 && in.gn_slabs && !in.save && g.K >= 512) {
      const hipError_t e = launch_gn_silu_splitk(s, g, ga, in.gn_slabs, in.gn_slices);
      if (e == hipSuccess) return prof_mark(h, s);
      (void)hipGetLastError();
      if (e != hipErrorInvalidValue) { set_error("launch_gn_silu_splitk failed: %s", hipGetErrorString(e)); return OSD_EHIP; }
    }
    OSD_HIP(launch_gn_silu(s, g, l.gw, ga));
    return prof_mark(h, s);
  };
  const float* cur = ws.h0;
  for (int b = 0; b < a.n_blocks; ++b) {
    OSD_TRY(layer(a.layers[2 * b], cur, ws.mid[b], ws.z1[b], ws.st1[b]));
    OSD_TRY(layer(a.layers[2 * b + 1], ws.mid[b], ws.out[b], ws.z2[b], ws.st2[b]));
    cur = ws.out[b];
  }
  return OSD_OK;
}

// Derived copies that follow the current parameters: the t_emb table time_proj(TimeEmbedding(t/T))
// (models/diffusion.py:222-223; all rows of a sampling step share t and training rows gather their
// t, so the Linear runs T times, not B) and the zero-padded input_proj.weight.
int refresh_derived(osd_handle* h, hipStream_t s, bool pack_in_w) {
  const Arch& a = h->arch;
  GemmArgs g{};
  g.A = h->params[a.pm.tp_w]; g.lda = a.time_dim; g.B0 = h->d_time_emb; g.ldb0 = a.time_dim; g.K0 = a.time_dim;
  g.F = a.H0; g.P = a.T; g.K = a.time_dim;
  OSD_HIP(launch_linear(s, g, true, true, h->params[a.pm.tp_b], h->d_temb, a.H0, false, false));
  h->panel_wpk_valid = false;           // the LDS-resident chain repacks its fragment-ordered copies before its next run
  h->squad_wpk_valid[0] = h->squad_wpk_valid[1] = false;      // ... and the squad chains theirs
  h->sq_wpk_t_fresh = false;
  h->split_valid = false;               // ... and the bf16x3 engine its weight planes
  if (!pack_in_w) {                     // a training step that reads input_proj.weight directly: the packed copies go stale and are
    h->w_packed_stale = true;           // refreshed by the next entry point that reads them (ensure_packed) or osd_load_weights
    return OSD_OK;
  }
  h->w_packed_stale = false;
  OSD_HIP(launch_copy2d(s, h->params[a.pm.in_w], a.D, h->w_in_packed, h->w_in_ld, a.H0, a.D));   // pad columns stay zero
  if (h->w_out_packed) {                       // D % 4 != 0: rows [D, Dp) stay zero
    const size_t hl = (size_t)a.block_out[a.n_blocks - 1];
    OSD_HIP(hipMemcpyAsync(h->w_out_packed, h->params[a.pm.out_w], (size_t)a.D * hl * 4, hipMemcpyDeviceToDevice, s));
    OSD_HIP(hipMemcpyAsync(h->b_out_packed, h->params[a.pm.out_b], (size_t)a.D * 4, hipMemcpyDeviceToDevice, s));
  }
  return OSD_OK;
}

// The packed input_proj / output_proj copies follow the parameters lazily: a training step that does not read them skips the
// repack (refresh_derived above), and a C-ABI caller may sample right after such a step without another osd_load_weights.
int ensure_packed(osd_handle* h, hipStream_t s) {
  if (!h->w_packed_stale) return OSD_OK;
  return refresh_derived(h, s, true);
}

// padded: the epilogue works on the padded chain state (Dp columns; the packed weight has zero rows for the pad columns)
GemmArgs output_proj_args(osd_handle* h, const FwdWs& ws, int64_t n, bool padded) {
  const Arch& a = h->arch;
  const int last = a.n_blocks - 1;
  GemmArgs g{};
  g.A = padded ? h->w_out_packed : h->params[a.pm.out_w]; g.lda = a.block_out[last];
  g.B0 = ws.out[last]; g.ldb0 = a.block_out[last]; g.K0 = a.block_out[last];
  g.F = padded ? h->Dp : a.D; g.P = (int)n; g.K = a.block_out[last];
  return g;
}

// The null condition of classifier-free guidance, host -> device slot (handle.h: null_cond) on the handle's stream.  The caller has
// checked that the vector is there and finite.
int upload_null_cond(osd_handle* h, int slot, const float* null_cond_host, const float** dev) {
  const int cd = h->arch.cond_dim;
  const size_t stride = (size_t)up64(cd);
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_TRY(h->null_cond.ensure(2 * stride));
  *dev = h->null_cond.dev() + slot * stride;
  // the vector rarely changes between calls (a training run, a generation run): the slot keeps what it holds and a call with the
  // same bits uploads nothing -- no host wait on the previous step, no copy on the hot stream
  if (h->null_valid[slot] && !memcmp(h->null_cond.host() + slot * stride, null_cond_host, (size_t)cd * 4)) return OSD_OK;
  float* host = nullptr;
  OSD_TRY(h->null_cond.staging(2 * stride, &host));
  h->null_valid[slot] = false;
  memcpy(host + slot * stride, null_cond_host, (size_t)cd * 4);
  OSD_TRY(h->null_cond.send(slot * stride, (size_t)cd, h->stream));
  h->null_valid[slot] = true;
  return OSD_OK;
}

int check_output_link(const osd_handle* h) {
  if (h->n_link > 0 && h->pred_type != OSD_PRED_SAMPLE) {
    set_error("output link (osd_set_output_link): %d logistic columns need the prediction type OSD_PRED_SAMPLE, the handle's is %d (osd_set_prediction)",
              h->n_link, h->pred_type);
    return OSD_EINVAL;
  }
  return OSD_OK;
}

int check_ready(osd_handle* h) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (!h->have_schedule) { set_error("osd_set_schedule has not been called"); return OSD_ESTATE; }
  if (!h->have_weights) { set_error("osd_load_weights has not been called"); return OSD_ESTATE; }
  return OSD_OK;
}

int check_rows(int64_t n) {
  if (n < 0 || n > 0x7fffffff / 2) { set_error("row count %lld out of range", (long long)n); return OSD_EINVAL; }
  return OSD_OK;
}

// Global row ids address the Philox stream as 32-bit counters: a shard whose ids would wrap would repeat another
// shard's draws, so it is rejected instead of truncated.
int check_row_offset(int64_t row_offset, int64_t n) {
  if (row_offset < 0 || row_offset + n > ((int64_t)1 << 32)) {
    set_error("row_offset %lld + %lld rows is outside the 32-bit global row id space [0, 2^32)", (long long)row_offset, (long long)n);
    return OSD_EINVAL;
  }
  return OSD_OK;
}

// Caller-supplied per-row timestep indices, clamped into [0, T) in a handle-owned buffer (see k_clamp_int).
int sanitize_t(osd_handle* h, hipStream_t s, const int32_t* t_index, int64_t n, const int** out) {
  if (!t_index) { *out = nullptr; return OSD_OK; }
  OSD_TRY(h->t_san.reserve((n + 1023) / 1024 * 1024, s));      // 1024-row granules
  OSD_HIP(launch_clamp_int(s, t_index, n, 0, h->arch.T - 1, h->t_san));
  *out = h->t_san;
  return OSD_OK;
}

// ---- shared by the chunk drivers (chain_chunk below, split.hip: split_chain_chunk) and the chain kernels' host files (fwd.h) ----
int release_graph(Slot& sl) {
  if (!sl.exec && !sl.graph) return OSD_OK;
  OSD_HIP(hipStreamSynchronize(sl.stream));
  sl.exec.reset();
  sl.graph.reset();
  return OSD_OK;
}

int chain_init_state(osd_handle* h, hipStream_t s, const ChainJob& job, float* x, int ldx, bool keep_aliased) {
  if (!job.x_T) OSD_HIP(launch_fill_randn(s, x, ldx, job.n, job.D, job.seed, (uint32_t)job.row_offset, (uint32_t)h->arch.T, TAG_POSTERIOR));
  else if (!(keep_aliased && job.x_T == x)) OSD_HIP(launch_copy2d(s, job.x_T, job.D, x, ldx, job.n, job.D));
  return OSD_OK;
}

// ---- osd_set_option / osd_get_option (include/osdiff.h documents each option) ----
template <class T, T osd_handle::*F> static void store_field(osd_handle* h, int64_t v) { h->*F = (T)v; }
template <class T, T osd_handle::*F> static int64_t load_field(osd_handle* h) { return (int64_t)(h->*F); }
#define OSD_FIELD(f) &store_field<decltype(osd_handle::f), &osd_handle::f>, &load_field<decltype(osd_handle::f), &osd_handle::f>

// A settable option: its values are [lo, hi], or -- n_only > 0 -- those of only[] within it; `err` is the message for any other
struct Option {
  const char* name;
  void (*store)(osd_handle*, int64_t);
  int64_t (*load)(osd_handle*);
  int64_t lo, hi;
  const char* err;
  int n_only;
  int64_t only[3];
};
static const Option OPTIONS[] = {
    {"chunk_rows", OSD_FIELD(chunk_rows), 1, INT64_MAX, "chunk_rows must be >= 1"},
    {"n_streams", OSD_FIELD(n_streams), 1, 8, "n_streams must be in [1,8]"},
    {"sampler", OSD_FIELD(sampler), 0, 2, "sampler must be 0 (auto), 1 (chain kernel) or 2 (per-layer kernels)"},
    {"train_squad", OSD_FIELD(train_squad), 0, 2,
     "train_squad must be 0 (per-layer launches), 1 (forward trunk as squads) or 2 (forward and the dgrad chain)"},
    {"squad_panel", OSD_FIELD(squad_panel), 0, 32, "squad_panel must be 0 (auto), 16 or 32", 3, {0, 16, 32}},
    {"chain_variant", OSD_FIELD(chain_variant), 0, 3,
     "chain_variant must be 0 (auto), 1 (workspace chain), 2 (LDS-resident chain) or 3 (squad chain)"},
    {"precision", OSD_FIELD(precision), 0, 1, "precision must be 0 (fp32) or 1 (bf16x3 split)"},
    {"chain_grid", OSD_FIELD(chain_grid), 0, 65536, "chain_grid must be in [0,65536]"},
    {"input_splitk", OSD_FIELD(input_splitk), -1, 64, "input_splitk must be in [-1,64]"},
    {"cond_bwd_fused", OSD_FIELD(cond_bwd_fused), 0, 1, "cond_bwd_fused must be 0 or 1"},
    {"chain_spin_budget", OSD_FIELD(chain_spin_budget), 0, INT64_MAX, "chain_spin_budget must be >= 0"},
    {"chain_wall_budget_ms", OSD_FIELD(chain_wall_budget_ms), 0, INT64_MAX, "chain_wall_budget_ms must be >= 0"},
    {"chain_steps_per_launch", OSD_FIELD(chain_steps_per_launch), 0, INT64_MAX, "chain_steps_per_launch must be >= 0"},
    {"chain_stagger", OSD_FIELD(chain_stagger), 0, 100000000, "chain_stagger must be in [0,1e8] cycles"},
    {"train_streams", OSD_FIELD(train_streams), 1, 2, "train_streams must be 1 or 2"},
    {"bound_rows", OSD_FIELD(bound_rows), 1, 0x7fffffff / 2, "bound_rows must be in [1, 2^30)"},
};
#undef OSD_FIELD

static const Option* find_option(const char* name) {
  for (const Option& o : OPTIONS)
    if (!strcmp(name, o.name)) return &o;
  return nullptr;
}

// read-only counters (osd_get_option only)
struct Counter { const char* name; int64_t (*load)(osd_handle*); };
static const Counter COUNTERS[] = {
    {"last_precision", [](osd_handle* h) -> int64_t { return h->last_precision; }},
    {"split_supported", [](osd_handle* h) -> int64_t { return split_supported(h->arch); }},
    {"chain_fallbacks", [](osd_handle* h) -> int64_t { return h->chain_fallbacks; }},
    {"last_engine", [](osd_handle* h) -> int64_t { return h->last_engine; }},
    {"last_chain_variant", [](osd_handle* h) -> int64_t { return h->last_chain_variant; }},
    {"panel_chain_supported", [](osd_handle* h) -> int64_t { return panel_chain_supported(h); }},
    {"squad_chain_supported", [](osd_handle* h) -> int64_t { return squad_chain_supported(h); }},
    {"last_squad_panel", [](osd_handle* h) -> int64_t { return h->last_squad_rp; }},
    {"last_train_path", [](osd_handle* h) -> int64_t { return h->last_train_path; }},
    {"prediction_type", [](osd_handle* h) -> int64_t { return h->pred_type; }},
    {"loss_mask", [](osd_handle* h) -> int64_t { return h->loss_mask ? 1 : 0; }},
    {"output_link", [](osd_handle* h) -> int64_t { return h->n_link; }},
};

}  // namespace osd

osd_handle::~osd_handle() {
  osd::split_free(this);
  osd::dp_free(this);
  osd::wgrad_group_free(this);
}

using namespace osd;

extern "C" {

int osd_version(void) { return OSD_VERSION; }
const char* osd_last_error(void) { return g_err; }

int osd_num_params(const osd_config* cfg) {
  if (!cfg) return 0;
  Arch a;
  if (build_arch(*cfg, &a) != OSD_OK) return 0;
  return a.pm.n_params;
}

int64_t osd_param_numel(const osd_config* cfg, int i) {
  if (!cfg) return -1;
  Arch a;
  if (build_arch(*cfg, &a) != OSD_OK) return -1;
  if (i < 0 || i >= a.pm.n_params) return -1;
  return a.pm.numel[i];
}

static int create_device_state(osd_handle* h) {
  const Arch& a = h->arch;
  const int T = a.T;
  OSD_TRY(h->d_sqrt_ac.reserve(T));
  OSD_TRY(h->d_sqrt_1m.reserve(T));
  OSD_TRY(h->d_coef.reserve((int64_t)T * 4));
  OSD_TRY(h->d_pq.reserve((int64_t)T * 2 * 2));      // (P, Q) [T][2], then osd_convert_prediction's (U, V) [T][2]
  const int64_t t_rows = ((int64_t)T + 31) / 32 * 32;     // zero rows up to whole K steps of the grouped weight-gradient kernel (time_proj.weight)
  OSD_TRY(h->d_time_emb.reserve(t_rows * a.time_dim));
  OSD_HIP(hipMemset(h->d_time_emb, 0, (size_t)t_rows * a.time_dim * 4));
  OSD_TRY(h->d_temb.reserve((int64_t)T * a.H0));
  h->w_in_ld = (a.D + BK - 1) / BK * BK;
  OSD_TRY(h->w_in_packed.reserve((int64_t)a.H0 * h->w_in_ld));
  OSD_HIP(hipMemset(h->w_in_packed, 0, (size_t)a.H0 * h->w_in_ld * 4));
  h->Dp = (a.D + 3) / 4 * 4;
  if (h->Dp != a.D) {
    const int64_t hl = a.block_out[a.n_blocks - 1];
    OSD_TRY(h->w_out_packed.reserve(h->Dp * hl));
    OSD_HIP(hipMemset(h->w_out_packed, 0, (size_t)h->Dp * hl * 4));
    OSD_TRY(h->b_out_packed.reserve(h->Dp));
    OSD_HIP(hipMemset(h->b_out_packed, 0, (size_t)h->Dp * 4));
  }
  OSD_TRY(h->main.t_dev.reserve(16));
  OSD_TRY(h->loss_dev.reserve(16));
  OSD_HIP(hipEventCreateWithFlags(h->fork_ev.put(), hipEventDisableTiming));
  return OSD_OK;
}

int osd_create(const osd_config* cfg, osd_handle** out) {
  if (!cfg || !out) { set_error("null argument"); return OSD_EINVAL; }
  *out = nullptr;
  Arch a;
  OSD_TRY(build_arch(*cfg, &a));
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no HIP device available: libosdiff has no CPU fallback"); return OSD_EHIP; }
  if (cfg->device < 0 || cfg->device >= ndev) { set_error("device %d out of range (%d devices)", cfg->device, ndev); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(cfg->device));
  OSD_HIP(prepare_kernels());
  osd_handle* h = new (std::nothrow) osd_handle();
  if (!h) { set_error("out of host memory"); return OSD_ENOMEM; }
  h->cfg = *cfg;
  h->arch = a;
  const int rc = create_device_state(h);
  if (rc != OSD_OK) {                 // nothing of a half-built handle survives (its members release what was allocated)
    osd_destroy(h);
    (void)hipGetLastError();          // the failed call's sticky error must not surface in a later launch check
    return rc;
  }
  *out = h;
  return OSD_OK;
}

int osd_destroy(osd_handle* h) {
  if (!h) return OSD_OK;
  hipError_t e = hipSetDevice(h->cfg.device);
  e = hipDeviceSynchronize();
  (void)e;
  delete h;
  return OSD_OK;
}

int osd_set_stream(osd_handle* h, void* hip_stream) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  h->stream = (hipStream_t)hip_stream;
  return OSD_OK;
}

int osd_set_option(osd_handle* h, const char* name, int64_t value) {
  if (!h || !name) { set_error("null argument"); return OSD_EINVAL; }
  const Option* o = find_option(name);
  if (!o) { set_error("unknown option '%s'", name); return OSD_EINVAL; }
  bool ok = value >= o->lo && value <= o->hi;
  if (ok && o->n_only) ok = std::find(o->only, o->only + o->n_only, value) != o->only + o->n_only;
  if (!ok) { set_error("%s", o->err); return OSD_EINVAL; }
  if (!strcmp(name, "precision") && value == 1 && !split_supported(h->arch)) {
    set_error("precision 1 (bf16x3 split) covers trunks of width 256 / 512 only");
    return OSD_EUNSUPPORTED;
  }
  o->store(h, value);
  return OSD_OK;
}

int osd_get_option(osd_handle* h, const char* name, int64_t* value) {
  if (!h || !name || !value) { set_error("null argument"); return OSD_EINVAL; }
  if (const Option* o = find_option(name)) { *value = o->load(h); return OSD_OK; }
  for (const Counter& c : COUNTERS)
    if (!strcmp(name, c.name)) { *value = c.load(h); return OSD_OK; }
  set_error("unknown option '%s'", name);
  return OSD_EINVAL;
}

// The per-step tables that depend on what the network predicts (osd_set_prediction), from the schedule scalars osd_set_schedule kept:
// d_coef (A, B, C, 0), sched_x0_coef (P, Q, E, F) and the device (P, Q) table of the constraint losses.  Every type's step is
// x' = E*x0 + F*x + C*z with x0 = P*x + Q*out; epsilon keeps the expressions it always had.
static int fold_schedule(osd_handle* h) {
  const Arch& a = h->arch;
  const float* post_coef = h->sched_post_coef.data();
  const int kind = h->pred_type;
  // fold the reference's six per-step scalars into x' = A*x + B*eps + C*z (see EpiPosterior)
  std::vector<float> abc((size_t)a.T * 4, 0.f);
  // ... and, for the chain that clips x0 (EpiPosterior<POST_CLIP>), the same scalars unfolded at x0: x0 = P*x + Q*eps, x' = E*x0 + F*x + C*z
  h->sched_x0_coef.assign((size_t)a.T * 4, 0.f);
  std::vector<float> pq((size_t)a.T * 2, 0.f);
  for (int t = 0; t < a.T; ++t) {
    const double c0 = post_coef[6 * t], c1 = post_coef[6 * t + 1], c2 = post_coef[6 * t + 2], c3 = post_coef[6 * t + 3],
                 c4 = post_coef[6 * t + 4], c5 = post_coef[6 * t + 5];
    float* r = &h->sched_x0_coef[4 * (size_t)t];
    r[2] = t > 0 ? (float)(c2 / c3) : 1.f;
    r[3] = t > 0 ? (float)(c4 / c3) : 0.f;
    abc[4 * t + 2] = t > 0 ? (float)c5 : 0.f;
    if (kind == OSD_PRED_EPSILON) {
      if (t > 0) {
        abc[4 * t] = (float)(c4 / c3 + c2 / (c1 * c3));
        abc[4 * t + 1] = (float)(-c0 * c2 / (c1 * c3));
      } else {
        abc[0] = (float)(1.0 / c1);
        abc[1] = (float)(-c0 / c1);
      }
      r[0] = (float)(1.0 / c1);
      r[1] = (float)(-c0 / c1);
      // what k_x0hat / k_x0hat_bwd compute in fp32 (they keep their own arithmetic for this type; the table is for osd_convert_prediction)
      pq[2 * t] = 1.f / h->sched_sqrt_ac[t];
      pq[2 * t + 1] = -(h->sched_sqrt_1m[t] / h->sched_sqrt_ac[t]);
      continue;
    }
    // a = sqrt_ac[t], b = sqrt_1m_ac[t]: the model's fp32 buffers
    const double sa = h->sched_sqrt_ac[t], sb = h->sched_sqrt_1m[t];
    const double P = kind == OSD_PRED_V ? sa : 0.0, Q = kind == OSD_PRED_V ? -sb : 1.0;
    const double E = t > 0 ? c2 / c3 : 1.0, F = t > 0 ? c4 / c3 : 0.0;
    abc[4 * t] = (float)(E * P + F);
    abc[4 * t + 1] = (float)(E * Q);
    r[0] = (float)P; r[1] = (float)Q;
    pq[2 * t] = (float)P; pq[2 * t + 1] = (float)Q;
  }
  OSD_HIP(hipMemcpy(h->d_coef, abc.data(), abc.size() * 4, hipMemcpyHostToDevice));
  OSD_HIP(hipMemcpy(h->d_pq, pq.data(), pq.size() * 4, hipMemcpyHostToDevice));
  h->conv_kind = -1;          // osd_convert_prediction's cached table belongs to the previous fold
  return OSD_OK;
}

int osd_set_schedule(osd_handle* h, const float* sqrt_ac, const float* sqrt_1m_ac, const float* post_coef, const float* time_emb) {
  if (!h || !sqrt_ac || !sqrt_1m_ac || !post_coef || !time_emb) { set_error("null argument"); return OSD_EINVAL; }
  const Arch& a = h->arch;
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_HIP(hipMemcpy(h->d_sqrt_ac, sqrt_ac, (size_t)a.T * 4, hipMemcpyHostToDevice));
  OSD_HIP(hipMemcpy(h->d_sqrt_1m, sqrt_1m_ac, (size_t)a.T * 4, hipMemcpyHostToDevice));
  h->sched_post_coef.assign(post_coef, post_coef + (size_t)a.T * 6);
  h->sched_sqrt_ac.assign(sqrt_ac, sqrt_ac + a.T);
  h->sched_sqrt_1m.assign(sqrt_1m_ac, sqrt_1m_ac + a.T);
  OSD_TRY(fold_schedule(h));
  OSD_HIP(hipMemcpy(h->d_time_emb, time_emb, (size_t)a.T * a.time_dim * 4, hipMemcpyHostToDevice));
  h->have_schedule = true;
  return OSD_OK;
}

int osd_load_weights(osd_handle* h, const float* const* params, int n) {
  if (!h || !params) { set_error("null argument"); return OSD_EINVAL; }
  const Arch& a = h->arch;
  if (n != a.pm.n_params) { set_error("expected %d parameter tensors, got %d", a.pm.n_params, n); return OSD_EINVAL; }
  if (!h->have_schedule) { set_error("osd_set_schedule must precede osd_load_weights"); return OSD_ESTATE; }
  for (int i = 0; i < n; ++i)
    if (!params[i]) { set_error("parameter %d is null", i); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  h->params.assign(params, params + n);
  OSD_TRY(refresh_derived(h, h->stream));
  h->have_weights = true;
  return OSD_OK;
}

// What both guided entry points refuse; *unguided: guidance_scale == 1 exactly -- the caller takes the unguided entry point's path.
static int check_guidance(osd_handle* h, const float* null_cond_host, float guidance_scale, int flags, bool* unguided) {
  if (!std::isfinite(guidance_scale)) { set_error("guidance_scale is not finite"); return OSD_EINVAL; }
  if (!null_cond_host) { set_error("null_cond is null"); return OSD_EINVAL; }
  for (int i = 0; i < h->arch.cond_dim; ++i)
    if (!std::isfinite(null_cond_host[i])) { set_error("null_cond[%d] is not finite", i); return OSD_EINVAL; }
  *unguided = guidance_scale == 1.0f;
  if (*unguided) return OSD_OK;
  if (flags & OSD_F_TRAIN_MODE) { set_error("guided sampling is eval mode only (no dropout inside a guided evaluation)"); return OSD_EINVAL; }
  if (h->precision == 1) { set_error("precision = bf16x3 does not run guided evaluations: set precision to fp32 or guidance_scale to 1"); return OSD_EUNSUPPORTED; }
  return OSD_OK;
}

// The condition batch of a guided chunk: the m rows' conditions and, as row m, the null condition -- so that c_proj of the null
// condition comes out of the same launches, with the bits it has as a row of any batch.  stage: [m + 1][cond_dim].
static int guided_cond(osd_handle* h, hipStream_t s, const Guide& gd, const float* cond, int64_t m, float* stage, const FwdWs& ws) {
  const int cd = h->arch.cond_dim;
  OSD_HIP(hipMemcpyAsync(stage, cond, (size_t)m * cd * 4, hipMemcpyDeviceToDevice, s));
  OSD_HIP(hipMemcpyAsync(stage + m * cd, gd.null_cond, (size_t)cd * 4, hipMemcpyDeviceToDevice, s));
  return run_cond(h, s, stage, m + 1, ws);
}

// A denoiser evaluation in the caller's terms: what osd_denoiser_forward and osd_denoiser_forward_guided receive, absent parts null.
struct ForwardRequest {
  const float* x; const int32_t* t_index; int32_t t_all; const float* cond; int64_t n; float* eps; int flags;
  const float* const* masks; uint64_t seed;
  bool guide;                     // check (and, unless guidance_scale == 1, apply) classifier-free guidance
  const float* null_cond; float guidance_scale;
};

// The one path of both entry points: a guided evaluation stages the null condition behind the batch's, runs the trunk on 2 n rows
// and combines the two halves in front of output_proj.
static int forward_request(osd_handle* h, const ForwardRequest& r) {
  const int64_t n = r.n;
  bool guided = r.guide;
  OSD_TRY(check_ready(h));
  if (guided) {
    bool unguided = false;
    OSD_TRY(check_guidance(h, r.null_cond, r.guidance_scale, r.flags, &unguided));
    guided = !unguided;
  }
  OSD_TRY(check_rows(n));
  if (!r.x || !r.cond || !r.eps) { set_error("null tensor"); return OSD_EINVAL; }
  const Arch& a = h->arch;
  if (!r.t_index && (r.t_all < 0 || r.t_all >= a.T)) { set_error("t=%d outside [0,%d)", r.t_all, a.T); return OSD_EINVAL; }
  if (n == 0) return OSD_OK;
  OSD_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  OSD_TRY(ensure_packed(h, s));
  const int* t_idx = nullptr;
  OSD_TRY(sanitize_t(h, s, r.t_index, n, &t_idx));
  Guide gd{nullptr, r.guidance_scale};
  if (guided) OSD_TRY(upload_null_cond(h, 0, r.null_cond, &gd.null_cond));
  if (h->precision == 1 && !(r.flags & OSD_F_TRAIN_MODE) && !r.masks) {      // eval mode on the bf16 matrix pipe; dropout stays fp32
    OSD_TRY(split_denoiser_forward(h, r.x, t_idx, r.t_all, r.cond, n, r.eps));
    if (r.flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(s));
    return OSD_OK;
  }
  h->last_precision = 0;
  const int64_t nt = guided ? 2 * n : n;        // rows of the trunk
  FwdWs ws;
  const int64_t need = up64(carve_fwd(a, nullptr, nt, false, &ws));
  OSD_TRY(h->main.arena.reserve(need + (guided ? (n + 1) * (int64_t)a.cond_dim : 0)));
  carve_fwd(a, h->main.arena, nt, false, &ws);
  if (guided) OSD_TRY(guided_cond(h, s, gd, r.cond, n, h->main.arena + need, ws));
  else OSD_TRY(run_cond(h, s, r.cond, n, ws));
  TrunkIn in{};
  in.x = r.x; in.ldx = a.D; in.n = nt; in.t_index = t_idx; in.t_imm = r.t_all;
  in.train = (r.flags & OSD_F_TRAIN_MODE) != 0; in.masks = r.masks; in.seed = r.seed;
  if (guided) { in.guide_m = n; in.cproj0 = ws.cproj + n * a.H0; }
  OSD_TRY(run_trunk(h, s, ws, in));
  if (guided) OSD_HIP(launch_guide_combine(s, ws.out[a.n_blocks - 1], n, a.block_out[a.n_blocks - 1], gd.w));
  GemmArgs g = output_proj_args(h, ws, n);
  OSD_HIP(launch_linear(s, g, true, true, h->params[a.pm.out_b], r.eps, a.D, false, false));
  if (r.flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

int osd_denoiser_forward(osd_handle* h, const float* x, const int32_t* t_index, int32_t t_all, const float* cond, int64_t n,
                         float* eps, int flags, const float* const* masks, uint64_t seed) {
  return forward_request(h, ForwardRequest{x, t_index, t_all, cond, n, eps, flags, masks, seed});
}

int osd_q_sample(osd_handle* h, const float* x0, const int32_t* t_index, const float* noise_in, int64_t n, uint64_t seed,
                 int64_t row_offset, float* x_t, float* noise_out) {
  if (!h || !h->have_schedule) { set_error("schedule not set"); return OSD_ESTATE; }
  OSD_TRY(check_rows(n));
  if (!x0 || !t_index || !x_t) { set_error("null tensor"); return OSD_EINVAL; }
  if (!noise_in && !noise_out) { set_error("noise_out is required when noise is generated"); return OSD_EINVAL; }
  OSD_TRY(check_row_offset(row_offset, n));
  OSD_HIP(hipSetDevice(h->cfg.device));
  const int* t_idx = nullptr;
  OSD_TRY(sanitize_t(h, h->stream, t_index, n, &t_idx));
  OSD_HIP(launch_q_sample(h->stream, x0, t_idx, h->d_sqrt_ac, h->d_sqrt_1m, noise_in, n, h->arch.D, seed, (uint32_t)row_offset, x_t, noise_out));
  return OSD_OK;
}

int osd_set_prediction(osd_handle* h, int type) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (type != OSD_PRED_EPSILON && type != OSD_PRED_V && type != OSD_PRED_SAMPLE) {
    set_error("unknown prediction type %d (OSD_PRED_EPSILON, OSD_PRED_V or OSD_PRED_SAMPLE)", type);
    return OSD_EINVAL;
  }
  if (!h->have_schedule) { set_error("osd_set_schedule must precede osd_set_prediction"); return OSD_ESTATE; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_HIP(hipDeviceSynchronize());       // chains in flight on the handle's own streams may still read the tables
  const int before = h->pred_type;
  h->pred_type = type;
  const int rc = fold_schedule(h);
  if (rc != OSD_OK) h->pred_type = before;
  return rc;
}

int osd_set_output_link(osd_handle* h, int n_logistic) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (n_logistic < 0 || n_logistic > h->arch.D) { set_error("n_logistic=%d outside [0, D=%d]", n_logistic, h->arch.D); return OSD_EINVAL; }
  if (n_logistic > 0 && h->pred_type != OSD_PRED_SAMPLE) {
    set_error("output link (osd_set_output_link): a logistic link needs osd_set_prediction(h, OSD_PRED_SAMPLE): the linked columns are x0^");
    return OSD_EINVAL;
  }
  h->n_link = n_logistic;      // host state alone: read when the next call is issued
  return OSD_OK;
}

int osd_q_sample_target(osd_handle* h, const float* x0, const int32_t* t_index, const float* noise_in, int64_t n, uint64_t seed,
                        int64_t row_offset, float* x_t, float* target_out) {
  if (!h || !h->have_schedule) { set_error("schedule not set"); return OSD_ESTATE; }
  if (h->pred_type == OSD_PRED_EPSILON && !h->loss_mask) {
    // the target is the noise: osd_q_sample, plus the copy it skips when the caller injected the noise
    OSD_TRY(osd_q_sample(h, x0, t_index, noise_in, n, seed, row_offset, x_t, noise_in ? nullptr : target_out));
    if (noise_in && target_out && target_out != noise_in && n > 0)
      OSD_HIP(hipMemcpyAsync(target_out, noise_in, (size_t)n * h->arch.D * 4, hipMemcpyDeviceToDevice, h->stream));
    return OSD_OK;
  }
  OSD_TRY(check_rows(n));
  if (!x0 || !t_index || !x_t || !target_out) { set_error("null tensor"); return OSD_EINVAL; }
  if (target_out == noise_in || target_out == x0 || target_out == x_t) { set_error("target_out must be a buffer of its own"); return OSD_EINVAL; }
  OSD_TRY(check_row_offset(row_offset, n));
  OSD_HIP(hipSetDevice(h->cfg.device));
  const int* t_idx = nullptr;
  OSD_TRY(sanitize_t(h, h->stream, t_index, n, &t_idx));
  OSD_HIP(launch_q_sample(h->stream, x0, t_idx, h->d_sqrt_ac, h->d_sqrt_1m, noise_in, n, h->arch.D, seed, (uint32_t)row_offset, x_t, target_out,
                          nullptr, 0, 0, nullptr, h->pred_type, h->loss_mask));
  return OSD_OK;
}

int osd_convert_prediction(osd_handle* h, const float* x_t, const int32_t* t_index, const float* out, int64_t n, int as_kind, float* dst) {
  if (!h || !h->have_schedule) { set_error("schedule not set"); return OSD_ESTATE; }
  OSD_TRY(check_rows(n));
  if (!x_t || !t_index || !out || !dst) { set_error("null tensor"); return OSD_EINVAL; }
  OSD_TRY(check_output_link(h));
  if (as_kind != OSD_PRED_EPSILON && as_kind != OSD_PRED_V && as_kind != OSD_PRED_SAMPLE) { set_error("unknown conversion %d (OSD_PRED_*)", as_kind); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  const int T = h->arch.T;
  float* uv_dev = h->d_pq + 2 * (size_t)T;
  if (h->conv_kind != as_kind) {
    std::vector<float> uv((size_t)T * 2);
    for (int t = 0; t < T; ++t) {
      const double a = h->sched_sqrt_ac[t], b = h->sched_sqrt_1m[t];
      const double P = h->pred_type == OSD_PRED_EPSILON ? 1.0 / a : h->pred_type == OSD_PRED_V ? a : 0.0;
      const double Q = h->pred_type == OSD_PRED_EPSILON ? -b / a : h->pred_type == OSD_PRED_V ? -b : 1.0;
      const double Ue = (1.0 - a * P) / b, Ve = -a * Q / b;      // eps^ = (x_t - a x0^) / b
      double U = P, V = Q;
      if (as_kind == OSD_PRED_EPSILON) { U = Ue; V = Ve; }
      if (as_kind == OSD_PRED_V) { U = a * Ue - b * P; V = a * Ve - b * Q; }
      uv[2 * t] = (float)U; uv[2 * t + 1] = (float)V;
    }
    OSD_HIP(hipStreamSynchronize(h->stream));      // an earlier conversion may still read the table
    OSD_HIP(hipMemcpy(uv_dev, uv.data(), uv.size() * 4, hipMemcpyHostToDevice));
    h->conv_kind = as_kind;
  }
  const int* t_idx = nullptr;
  OSD_TRY(sanitize_t(h, h->stream, t_index, n, &t_idx));
  // osd_set_output_link: x0^ is sigma(out) on the link columns, eps^ and v^ follow from that x0^ (k_train.hip: k_row_affine)
  OSD_HIP(launch_row_affine(h->stream, x_t, t_idx, reinterpret_cast<const float2*>(uv_dev), out, n, h->arch.D, dst, h->n_link));
  return OSD_OK;
}

int osd_p_sample_step(osd_handle* h, const float* x_t, int32_t t, const float* cond, const float* z, int64_t n, uint64_t seed,
                      int64_t row_offset, float* x_out, int flags) {
  OSD_TRY(check_ready(h));
  OSD_TRY(check_rows(n));
  if (!x_t || !cond || !x_out) { set_error("null tensor"); return OSD_EINVAL; }
  if (h->n_link > 0) {
    set_error("output link (osd_set_output_link): osd_p_sample_step folds x0^ away and cannot carry the link; osd_sample_chain_clipped does");
    return OSD_EUNSUPPORTED;
  }
  const Arch& a = h->arch;
  if (t < 0 || t >= a.T) { set_error("t=%d outside [0,%d)", t, a.T); return OSD_EINVAL; }
  OSD_TRY(check_row_offset(row_offset, n));
  if (n == 0) return OSD_OK;
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_TRY(ensure_packed(h, h->stream));
  if (h->precision == 1 && !((flags & OSD_F_TRAIN_MODE) && h->cfg.dropout_p > 0.f)) {
    OSD_TRY(split_p_sample_step(h, x_t, t, cond, z, n, seed, row_offset, x_out));
    if (flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(h->stream));
    return OSD_OK;
  }
  h->last_precision = 0;
  FwdWs ws;
  const int64_t need = carve_fwd(a, nullptr, n, false, &ws);
  OSD_TRY(h->main.arena.reserve(need));
  carve_fwd(a, h->main.arena, n, false, &ws);
  hipStream_t s = h->stream;
  OSD_TRY(run_cond(h, s, cond, n, ws));      // recomputed every step, as models/diffusion.py:395 does
  TrunkIn in{};
  in.x = x_t; in.ldx = a.D; in.n = n; in.t_imm = t;
  in.train = (flags & OSD_F_TRAIN_MODE) != 0; in.seed = seed; in.row_offset = (uint32_t)row_offset; in.drop_step = (uint32_t)t;
  OSD_TRY(run_trunk(h, s, ws, in));
  GemmArgs g = output_proj_args(h, ws, n);
  PosteriorArgs ea{};
  ea.bias = h->params[a.pm.out_b]; ea.xin = x_t; ea.ldx = a.D; ea.xout = x_out; ea.ldo = a.D; ea.coef = h->d_coef;
  ea.t_dev = nullptr; ea.t_imm = t; ea.z = z; ea.ldzz = a.D; ea.z_step_stride = 0; ea.t_first = t;
  ea.seed = seed; ea.row_offset = (uint32_t)row_offset; ea.mut_mask = nullptr; ea.mutation_dim = 0;
  OSD_HIP(launch_posterior(s, g, ea));
  if (flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}

// One chunk of the reverse chain on one slot: rows [r0, r0+m).  A guided chain runs the trunk on 2 m rows (rows [0, m) with the
// patients' conditions, [m, 2 m) with the null condition), input_proj and output_proj on m.
static int chain_chunk(osd_handle* h, const ChainJob& whole, Slot& sl, int64_t r0, int64_t m) {
  const Arch& a = h->arch;
  const ChainJob job = whole.chunk(r0, m);
  const Guide* gd = job.guide.null_cond ? &job.guide : nullptr;
  const Known* kn = job.known.known ? &job.known : nullptr;
  const Clip* cl = job.clip.bounds ? &job.clip : nullptr;
  const Multistep* ms = job.multistep.hist_coef ? &job.multistep : nullptr;
  const int D = a.D, S = job.plan.n_steps;
  hipStream_t s = sl.stream;
  OSD_TRY(release_graph(sl));
  FwdWs ws;
  const int64_t mt = gd ? 2 * m : m;            // rows of the trunk
  const int64_t need = carve_fwd(a, nullptr, mt, false, &ws);
  // D % 4 != 0 with device-generated draws: the state of the chunk lives in a padded buffer behind the activations (rows of Dp
  // floats, pad columns zero at the start) and is copied to the caller's rows at the end; injected draws ([S-1][n][D], rows not
  // 16-byte aligned) keep the guarded kernels on the caller's tensor
  const bool padded = h->w_out_packed != nullptr && !job.noises;
  const int ldx = padded ? h->Dp : D;
  const int64_t need_pad = up64(need);
  // small batches: input_proj split-K (k_fused.hip) -- few output tiles, each a long sequential K loop
  int in_slices = 0;
  constexpr int64_t INPUT_SPLITK_TARGET = 768;      // workgroups the auto mode (-1) aims at: slices = this / output tiles
  {
    const int64_t tiles = (int64_t)((a.H0 + 63) / 64) * ((m + 63) / 64);
    if (h->input_splitk > 0 && !h->splitk_suspended) in_slices = h->input_splitk;
    else if (h->input_splitk < 0 && !h->splitk_suspended && ldx >= 1024 && tiles < 384)      // fewer tiles than 1.5 per CU
      in_slices = (int)std::min<int64_t>(16, std::max<int64_t>(2, (INPUT_SPLITK_TARGET + tiles / 2) / tiles));
    in_slices = std::min(in_slices, ldx / 128);
    if (in_slices < 2) in_slices = 0;
  }
  const int64_t x_floats = padded ? up64(m * (int64_t)ldx) : 0;
  // ... and the deep Linear+GroupNorm layers likewise (same switch: the small-batch mode): slices so that a 512-wide layer has ~640
  // workgroups (64 x 64 tiles)
  int gn_slices = 0, max_c = a.H0;
  for (int c : a.block_out) max_c = std::max(max_c, c);
  if (in_slices > 0 && !(job.flags & OSD_F_TRAIN_MODE)) {
    const int64_t tiles = (int64_t)((max_c + 63) / 64) * ((mt + 63) / 64);
    gn_slices = (int)std::min<int64_t>(4, (640 + tiles / 2) / tiles);
    if (gn_slices < 4) gn_slices = 0;      // measured (dims 62 / 5054 / 26): 999 rows 257 -> 238 us per step with 4 slices; 3000 rows 351 -> 385 us with 2
  }
  // a guided chunk in the small-batch mode: input_proj split over K as for m rows (its reduce kernel writes both halves), the deep
  // layers' K slices and the two-wave-group GEMMs as for 2 m unguided rows.  The slabs end on a 64-float boundary so that whatever is
  // carved behind them (a guided chunk's condition staging) stays aligned
  const int64_t slab_floats = up64(std::max<int64_t>((int64_t)in_slices * m * a.H0, gn_slices ? (int64_t)(gn_slices + 1) * mt * max_c : 0));
  const int64_t stage_floats = gd ? (m + 1) * (int64_t)a.cond_dim : 0;
  // a padded state reads its observations from rows of Dp floats too: the chunk's known rows, copied once, pad columns NaN (free)
  const int64_t known_floats = kn && padded ? m * (int64_t)ldx : 0;
  // a multistep chain keeps the previous step's clipped x0 beside the state: rows of ldx floats like the state's, zero at the start
  const int64_t hist_floats = ms ? m * (int64_t)ldx : 0;
  OSD_TRY(sl.arena.reserve(need_pad + x_floats + slab_floats + up64(stage_floats) + (ms ? up64(known_floats) : known_floats) + hist_floats));
  carve_fwd(a, sl.arena, mt, false, &ws);
  float* x = padded ? sl.arena + need_pad : job.x_out;       // else the chain state lives in the output rows
  float* in_slabs = in_slices ? sl.arena + need_pad + x_floats : nullptr;
  float* cond_stage = sl.arena + need_pad + x_floats + slab_floats;
  if (padded) OSD_HIP(hipMemsetAsync(x, 0, (size_t)m * ldx * 4, s));
  const float* known = job.known.known;
  int ldk = (int)job.known.ld;
  if (kn && padded) {
    float* kpad = cond_stage + up64(stage_floats);
    OSD_HIP(hipMemsetAsync(kpad, 0xff, (size_t)m * ldx * 4, s));          // all bits set: a NaN
    OSD_HIP(launch_copy2d(s, known, ldk, kpad, ldx, m, D));
    known = kpad; ldk = ldx;
  }
  float* hist = nullptr;
  if (ms) {
    hist = cond_stage + up64(stage_floats) + up64(known_floats);
    OSD_HIP(hipMemsetAsync(hist, 0, (size_t)m * ldx * 4, s));
  }
  const uint32_t roff = (uint32_t)job.row_offset;
  const bool train = (job.flags & OSD_F_TRAIN_MODE) != 0;
  // conditioning is loop-invariant in eval mode (no dropout inside the embedding MLP): hoisted
  if (gd) OSD_TRY(guided_cond(h, s, *gd, job.cond, m, cond_stage, ws));
  else OSD_TRY(run_cond(h, s, job.cond, m, ws));
  OSD_TRY(chain_init_state(h, s, job, x, ldx, false));

  OSD_TRY(run_steps(sl, S, job.flags, [&](void) -> int {
    TrunkIn in{};
    in.x = x; in.ldx = ldx; in.kx = ldx; in.n = mt; in.t_dev = sl.t_dev; in.temb = job.plan.temb; in.in_slabs = in_slabs; in.in_slices = in_slices;
    if (gd) { in.guide_m = m; in.cproj0 = ws.cproj + m * a.H0; }
    in.gn_slabs = in_slabs; in.gn_slices = gn_slices;
    in.ksplit = in_slices > 1;             // the small-batch mode already trades bit-equality with the chain kernel for latency: long-K layers on two wave groups
    in.train = train; in.seed = job.seed; in.row_offset = roff; in.drop_step_dev = sl.t_dev;
    OSD_TRY(run_trunk(h, s, ws, in));
    // guidance on the last hidden activation, in place over the conditional rows: output_proj + posterior then run once, on m rows
    if (gd) OSD_HIP(launch_guide_combine(s, ws.out[a.n_blocks - 1], m, a.block_out[a.n_blocks - 1], gd->w));
    GemmArgs g = output_proj_args(h, ws, m, padded);
    PosteriorArgs ea{};
    ea.bias = padded ? h->b_out_packed : h->params[a.pm.out_b]; ea.xin = x; ea.ldx = ldx; ea.xout = x; ea.ldo = ldx; ea.coef = job.plan.coef;
    ea.t_dev = sl.t_dev; ea.t_imm = 0;
    ea.z = job.noises; ea.ldzz = D; ea.z_step_stride = (long long)job.n_total * D; ea.t_first = S - 1;
    ea.seed = job.seed; ea.row_offset = roff;
    ea.mut_mask = job.mut_mask_out; ea.mutation_dim = job.mutation_dim;
    if (cl) {
      const PosteriorClipArgs ca{ea, cl->bounds, cl->bounds + cl->ld, cl->x0_coef, kn ? known : nullptr, ldk, kn ? kn->level : nullptr};
      if (cl->n_link > 0) {            // osd_set_output_link: the same launch, sigma on the leading columns of x0^
        if (ms) OSD_HIP(launch_posterior(s, g, PosteriorHistLinkArgs{PosteriorHistArgs{ca, hist, ldx, ms->hist_coef}, cl->n_link}));
        else OSD_HIP(launch_posterior(s, g, PosteriorClipLinkArgs{ca, cl->n_link}));
      } else if (ms) OSD_HIP(launch_posterior(s, g, PosteriorHistArgs{ca, hist, ldx, ms->hist_coef}));
      else OSD_HIP(launch_posterior(s, g, ca));
    } else if (kn) OSD_HIP(launch_posterior(s, g, PosteriorKnownArgs{ea, known, ldk, kn->level}));
    else OSD_HIP(launch_posterior(s, g, ea));
    OSD_HIP(launch_add_int(s, sl.t_dev, -1));
    return OSD_OK;
  }));
  if (padded) OSD_HIP(launch_copy2d(s, x, ldx, job.x_out, D, m, D));
  return OSD_OK;
}

// The reverse chain of one validated request: sample_request after its argument checks, chain_check_status and ensure_packed.
static int sample_plan(osd_handle* h, const ChainJob& job) {
  const int64_t n = job.n;
  const int flags = job.flags;
  const bool gd = job.guide.null_cond != nullptr, kn = job.known.known != nullptr, cl = job.clip.bounds != nullptr;
  // bf16x3 split precision: eval-mode chains on the per-layer launches of split.hip (dropout inside the chain stays fp32)
  const bool split = !gd && !kn && !cl && h->precision == 1 && !((flags & OSD_F_TRAIN_MODE) && h->cfg.dropout_p > 0.f);
  h->last_precision = split ? 1 : 0;
  if (split) OSD_TRY(split_pack_weights(h, h->stream));
  // a guided chain runs on the per-layer kernels whatever "sampler" says: the chain kernels' tiles are sized for m trunk rows; so does
  // a chain around known values or one that clips x0, whose epilogues only the per-layer output_proj launch has
  h->last_engine = (split || gd || kn || cl) ? 0 : chain_pick_engine(h, n, flags);
  if (h->last_engine == 1 && job.noises && h->w_out_packed && !chain_uses_squad(h, n)) h->last_engine = 0;      // injected draws at D % 4 != 0: guarded per-layer kernels (the squad chain reads any layout)
  bool fell_back = false;
  if (h->last_engine == 1) {
    OSD_TRY(chain_run(h, job));
    if (!(flags & OSD_F_SYNC)) return OSD_OK;       // asynchronous: a chain that gives up is reported by the next call on this handle
    int gave_up = 0;
    OSD_TRY(chain_finish(h, &gave_up));
    if (!gave_up) return OSD_OK;
    // models/diffusion.py:427-449 cannot fail: the chain is re-run on the per-layer kernels, which compute the same bits from
    // the same x_T / seed (the chain state lives in x_out, so an aliased x_T is gone)
    if (job.x_T == job.x_out) {
      set_error("the reverse-chain kernel gave up and x_T aliases x_out: nothing left to re-run the chain from");
      return OSD_EHIP;
    }
    ++h->chain_fallbacks;
    h->last_engine = 0;
    fell_back = true;
    h->splitk_suspended = true;          // the re-run must produce the chain kernel's bits: single-pass input_proj
  }
  // equal chunks (rounded up to whole 128-row tiles) of at most chunk_rows rows
  int64_t n_chunks = (n + h->chunk_rows - 1) / h->chunk_rows;
  int64_t chunk = ((n + n_chunks - 1) / n_chunks + 127) / 128 * 128;
  if (chunk > n) chunk = n;
  n_chunks = (n + chunk - 1) / chunk;
  const int n_slots = (int)std::min<int64_t>(h->n_streams, n_chunks);
  while ((int)h->slots.size() < n_slots) {
    Slot sl;
    OSD_HIP(hipStreamCreateWithFlags(sl.stream.put(), hipStreamNonBlocking));
    OSD_HIP(hipEventCreateWithFlags(sl.done.put(), hipEventDisableTiming));
    OSD_TRY(sl.t_dev.reserve(16));
    h->slots.push_back(std::move(sl));
  }
  // fork: slot streams wait for everything already queued on the caller's stream
  OSD_HIP(hipEventRecord(h->fork_ev, h->stream));
  for (int i = 0; i < n_slots; ++i) OSD_HIP(hipStreamWaitEvent(h->slots[i].stream, h->fork_ev, 0));
  int rc = OSD_OK;
  for (int64_t c = 0; c < n_chunks && rc == OSD_OK; ++c) {
    const int64_t r0 = c * chunk;
    const int64_t m = std::min<int64_t>(chunk, n - r0);
    rc = split ? split_chain_chunk(h, job, h->slots[c % n_slots], r0, m) : chain_chunk(h, job, h->slots[c % n_slots], r0, m);
  }
  // join
  for (int i = 0; i < n_slots; ++i) {
    hipError_t e = hipEventRecord(h->slots[i].done, h->slots[i].stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->slots[i].done, 0);
    if (e != hipSuccess && rc == OSD_OK) { set_error("join failed: %s", hipGetErrorString(e)); rc = OSD_EHIP; }
  }
  h->splitk_suspended = false;
  if (rc != OSD_OK) return rc;
  if (flags & OSD_F_SYNC) OSD_HIP(hipStreamSynchronize(h->stream));
  if (fell_back)       // a warning, not an error: osd_last_error() tells what happened, osd_get_option("chain_fallbacks") counts
    set_error("warning: the reverse-chain kernel gave up in a dependency wait; the chain was re-run on the per-layer kernels (%s)",
              h->last_chain_variant == 3 ? "results agree with the squad chain's to fp32 rounding" : "same results");
  return OSD_OK;
}

// The tables of osd_sample_chain_steps' plan, on the handle's stream: coefficients and timesteps uploaded through the handle's
// staging, temb rows gathered from d_temb (which ensure_packed has just brought up to date with the parameters).  An earlier call's
// chunks on the slot streams have joined h->stream, so nothing still reads the tables this overwrites.
static int upload_plan(osd_handle* h, const int32_t* timesteps, const float* step_coef, int S, StepPlan* out) {
  const Arch& a = h->arch;
  hipStream_t s = h->stream;
  OSD_TRY(h->plan_temb.reserve((int64_t)a.T * a.H0));
  float* hc = nullptr;
  OSD_TRY(h->plan_tab.staging((size_t)a.T * 5, &hc));          // [S][4] coefficients, then [S] timesteps
  if (step_coef) memcpy(hc, step_coef, (size_t)S * 4 * 4);
  else memset(hc, 0, (size_t)S * 4 * 4);           // a multistep plan: no step draws, and its launch reads (P, Q, G, F) and H instead
  memcpy(hc + (size_t)S * 4, timesteps, (size_t)S * 4);
  OSD_TRY(h->plan_tab.send(0, (size_t)S * 5, s));
  OSD_HIP(launch_gather_rows(s, h->d_temb, a.H0, reinterpret_cast<const int*>(h->plan_tab.dev() + (size_t)S * 4), S, h->plan_temb));
  *out = StepPlan{S, h->plan_temb, h->plan_tab.dev()};
  return OSD_OK;
}

// What every entry point that takes a step plan rejects in it.
static int check_plan(const Arch& a, const int32_t* timesteps, const float* step_coef, int32_t n_steps, bool need_coef = true) {
  if (!timesteps || (need_coef && !step_coef)) { set_error("null step plan"); return OSD_EINVAL; }
  if (n_steps < 1 || n_steps > a.T) { set_error("n_steps=%d outside [1,%d]", n_steps, a.T); return OSD_EINVAL; }
  for (int s = 0; s < n_steps; ++s) {
    if (timesteps[s] < 0 || timesteps[s] >= a.T) { set_error("timesteps[%d]=%d outside [0,%d)", s, timesteps[s], a.T); return OSD_EINVAL; }
    for (int k = 0; step_coef && k < 4; ++k)
      if (!std::isfinite(step_coef[4 * s + k])) { set_error("step_coef[%d] is not finite", 4 * s + k); return OSD_EINVAL; }
  }
  if (step_coef && step_coef[2] != 0.f) { set_error("step_coef[2] = C_0 = %g: the last step draws no z, so C_0 must be 0", (double)step_coef[2]); return OSD_EINVAL; }
  return OSD_OK;
}

// The level table of a chain around known values, host -> handle-owned device table on the handle's stream.  level_host: the plan's
// [S][2], or null for the DDPM identity plan, whose rows are the schedule's own: (sqrt_ac[s - 1], sqrt_1m_ac[s - 1]), (1, 0) at s = 0.
static int upload_known_level(osd_handle* h, const float* level_host, int S, const float** dev) {
  float* hl = nullptr;
  OSD_TRY(h->known_level.staging((size_t)h->arch.T * 2, &hl));
  if (level_host) {
    memcpy(hl, level_host, (size_t)S * 2 * 4);
  } else {
    hl[0] = 1.f; hl[1] = 0.f;
    for (int s = 1; s < S; ++s) { hl[2 * s] = h->sched_sqrt_ac[s - 1]; hl[2 * s + 1] = h->sched_sqrt_1m[s - 1]; }
  }
  OSD_TRY(h->known_level.send(0, (size_t)S * 2, h->stream));
  *dev = h->known_level.dev();
  return OSD_OK;
}

// The two tables of a chain that clips x0, host -> one handle-owned device buffer on the handle's stream: coefficients [S][4] -- the
// plan's, or null for the DDPM chain, whose rows osd_set_schedule folded --, then the bounds as two rows of Dp floats whose pad columns
// are (-inf, +inf): a padded chain state and the caller's rows read the same rows.
static int upload_clip(osd_handle* h, const float* x0_coef_host, int S, const float* lo_host, const float* hi_host, Clip* out) {
  const Arch& a = h->arch;
  const size_t coef_floats = (size_t)up64((int64_t)a.T * 4), floats = coef_floats + 2 * (size_t)h->Dp;
  float* hc = nullptr;
  OSD_TRY(h->clip_tab.staging(floats, &hc));
  memcpy(hc, x0_coef_host ? x0_coef_host : h->sched_x0_coef.data(), (size_t)S * 4 * 4);
  float* lo = hc + coef_floats;
  float* hi = lo + h->Dp;
  if (lo_host) memcpy(lo, lo_host, (size_t)a.D * 4);
  if (hi_host) memcpy(hi, hi_host, (size_t)a.D * 4);
  for (int f = lo_host ? a.D : 0; f < h->Dp; ++f) { lo[f] = -INFINITY; hi[f] = INFINITY; }      // no bounds (a multistep chain's may be absent): all free
  OSD_TRY(h->clip_tab.send(0, floats, h->stream));
  *out = Clip{h->clip_tab.dev() + coef_floats, h->Dp, h->clip_tab.dev(), 0};
  return OSD_OK;
}

// The history coefficients of a multistep chain, host -> handle-owned device table on the handle's stream.
static int upload_hist_coef(osd_handle* h, const float* hist_coef_host, int S, Multistep* out) {
  float* hh = nullptr;
  OSD_TRY(h->hist_coef.staging((size_t)h->arch.T, &hh));
  memcpy(hh, hist_coef_host, (size_t)S * 4);
  OSD_TRY(h->hist_coef.send(0, (size_t)S, h->stream));
  *out = Multistep{h->hist_coef.dev()};
  return OSD_OK;
}

// A reverse-chain request in the caller's terms: what the osd_sample_chain* entry points receive, absent parts null.
struct SampleRequest {
  const float* cond; int64_t n; const float* x_T; const float* noises; uint64_t seed; int64_t row_offset;
  float* x_out; float* mut_mask_out; int flags;
  bool need_plan;                 // osd_sample_chain_steps: a step plan is required; elsewhere timesteps == null means the DDPM chain
  const int32_t* timesteps; const float* step_coef; int32_t n_steps;
  bool guide;                     // check (and, unless guidance_scale == 1, apply) classifier-free guidance
  const float* null_cond; float guidance_scale;
  bool around_known;              // osd_sample_chain_known
  const float* known; int64_t ld_known; const float* known_level;
  bool clipped;                   // osd_sample_chain_clipped
  const float* x0_coef; const float* lo; const float* hi;
  bool multistep;                 // osd_sample_chain_multistep: clipped, with no step_coef, optional bounds and hist_coef [n_steps]
  const float* hist_coef;
};

// The one path of the osd_sample_chain* entry points: validation (in the order the entry points document: the first bad argument
// names the error), the device prologue, the request's uploads, the chain.
static int sample_request(osd_handle* h, const SampleRequest& r) {
  OSD_TRY(check_ready(h));
  const Arch& a = h->arch;
  bool unguided = true;
  if (r.guide) OSD_TRY(check_guidance(h, r.null_cond, r.guidance_scale, r.flags, &unguided));
  if (r.around_known && h->precision == 1) { set_error("precision = bf16x3 does not run chains around known values: set precision to fp32"); return OSD_EUNSUPPORTED; }
  if (r.multistep && h->precision == 1) { set_error("precision = bf16x3 does not run the multistep solver: set precision to fp32"); return OSD_EUNSUPPORTED; }
  if (r.clipped && h->precision == 1) { set_error("precision = bf16x3 does not run chains that clip x0: set precision to fp32"); return OSD_EUNSUPPORTED; }
  if (h->n_link > 0) {
    OSD_TRY(check_output_link(h));
    if (!r.clipped) {
      set_error("output link (osd_set_output_link): this entry point folds x0^ away and cannot carry the link; osd_sample_chain_clipped and "
                "osd_sample_chain_multistep do (infinite bounds leave a column free)");
      return OSD_EUNSUPPORTED;
    }
  }
  OSD_TRY(check_rows(r.n));
  if (!r.cond || !r.x_out) { set_error("null tensor"); return OSD_EINVAL; }
  if (r.around_known) {
    if (!r.known) { set_error("known is null"); return OSD_EINVAL; }
    if (r.ld_known < a.D || r.ld_known > 0x7fffffff) { set_error("ld_known=%lld outside [D=%d, 2^31)", (long long)r.ld_known, a.D); return OSD_EINVAL; }
  }
  const bool plan = r.need_plan || r.timesteps;
  if (plan) OSD_TRY(check_plan(a, r.timesteps, r.step_coef, r.n_steps, !r.multistep));
  if (plan && r.around_known) {
    if (!r.known_level) { set_error("null known_level"); return OSD_EINVAL; }
    for (int i = 0; i < 2 * r.n_steps; ++i)
      if (!std::isfinite(r.known_level[i])) { set_error("known_level[%d] is not finite", i); return OSD_EINVAL; }
    if (r.known_level[0] != 1.f || r.known_level[1] != 0.f) {
      set_error("known_level[0] = (%g, %g): the last step returns the observations themselves, so it must be (1, 0)", (double)r.known_level[0], (double)r.known_level[1]);
      return OSD_EINVAL;
    }
  }
  if (r.clipped) {
    const bool unbounded = r.multistep && !r.lo && !r.hi;
    if (!unbounded && (!r.lo || !r.hi)) { set_error("null bound"); return OSD_EINVAL; }
    for (int f = 0; !unbounded && f < a.D; ++f) {
      if (std::isnan(r.lo[f]) || std::isnan(r.hi[f])) { set_error("bound %d is NaN", f); return OSD_EINVAL; }
      if (r.lo[f] > r.hi[f]) { set_error("lo[%d] = %g > hi[%d] = %g", f, (double)r.lo[f], f, (double)r.hi[f]); return OSD_EINVAL; }
    }
    if (plan) {
      if (!r.x0_coef) { set_error("null x0_coef"); return OSD_EINVAL; }
      for (int i = 0; i < 4 * r.n_steps; ++i)
        if (!std::isfinite(r.x0_coef[i])) { set_error("x0_coef[%d] is not finite", i); return OSD_EINVAL; }
      if (r.x0_coef[2] != 1.f || r.x0_coef[3] != 0.f) {
        set_error("x0_coef[0] = (., ., %g, %g): the last step returns the clipped x0 itself, so E_0, F_0 must be (1, 0)", (double)r.x0_coef[2], (double)r.x0_coef[3]);
        return OSD_EINVAL;
      }
    }
  }
  if (r.multistep) {
    if (!r.hist_coef) { set_error("null hist_coef"); return OSD_EINVAL; }
    for (int i = 0; i < r.n_steps; ++i)
      if (!std::isfinite(r.hist_coef[i])) { set_error("hist_coef[%d] is not finite", i); return OSD_EINVAL; }
    if (r.hist_coef[0] != 0.f || r.hist_coef[r.n_steps - 1] != 0.f) {
      set_error("hist_coef[0] = %g, hist_coef[%d] = %g: the last step is first order and the first one has no history, so both must be 0",
                (double)r.hist_coef[0], r.n_steps - 1, (double)r.hist_coef[r.n_steps - 1]);
      return OSD_EINVAL;
    }
  }
  OSD_TRY(check_row_offset(r.row_offset, r.n));
  if (r.n == 0) return OSD_OK;
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_TRY(chain_check_status(h));            // a previous chain-kernel run that gave up is reported here at the latest
  OSD_TRY(ensure_packed(h, h->stream));
  ChainJob job{};
  job.plan = StepPlan{a.T, h->d_temb, h->d_coef};
  job.cond = r.cond; job.n = job.n_total = r.n; job.x_T = r.x_T; job.noises = r.noises; job.seed = r.seed; job.row_offset = r.row_offset;
  job.x_out = r.x_out; job.mut_mask_out = r.mut_mask_out; job.flags = r.flags;
  job.D = a.D; job.cond_dim = a.cond_dim; job.mutation_dim = h->cfg.mutation_dim;
  job.guide.w = r.guidance_scale;
  if (!unguided) OSD_TRY(upload_null_cond(h, 0, r.null_cond, &job.guide.null_cond));
  if (r.around_known) {
    job.known.known = r.known; job.known.ld = r.ld_known;
    OSD_TRY(upload_known_level(h, plan ? r.known_level : nullptr, plan ? r.n_steps : a.T, &job.known.level));
  }
  if (r.clipped) OSD_TRY(upload_clip(h, plan ? r.x0_coef : nullptr, plan ? r.n_steps : a.T, r.lo, r.hi, &job.clip));
  job.clip.n_link = h->n_link;
  if (r.multistep) OSD_TRY(upload_hist_coef(h, r.hist_coef, r.n_steps, &job.multistep));
  if (plan) OSD_TRY(upload_plan(h, r.timesteps, r.step_coef, r.n_steps, &job.plan));
  return sample_plan(h, job);
}

int osd_sample_chain(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                     int64_t row_offset, float* x_out, float* mut_mask_out, int flags) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags};
  return sample_request(h, r);
}

int osd_sample_chain_steps(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                           int64_t row_offset, float* x_out, float* mut_mask_out, int flags, const int32_t* timesteps,
                           const float* step_coef, int32_t n_steps) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags, true, timesteps, step_coef, n_steps};
  return sample_request(h, r);
}

int osd_sample_chain_guided(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                            int64_t row_offset, float* x_out, float* mut_mask_out, int flags, const int32_t* timesteps,
                            const float* step_coef, int32_t n_steps, const float* null_cond_host, float guidance_scale) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags, false, timesteps, step_coef, n_steps,
                  true, null_cond_host, guidance_scale};
  return sample_request(h, r);
}

int osd_sample_chain_known(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                           int64_t row_offset, float* x_out, float* mut_mask_out, int flags, const int32_t* timesteps,
                           const float* step_coef, const float* known_level, int32_t n_steps, const float* null_cond_host,
                           float guidance_scale, const float* known, int64_t ld_known) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags, false, timesteps, step_coef, n_steps,
                  null_cond_host != nullptr, null_cond_host, guidance_scale, true, known, ld_known, known_level};
  return sample_request(h, r);
}

int osd_sample_chain_clipped(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                             int64_t row_offset, float* x_out, float* mut_mask_out, int flags, const int32_t* timesteps,
                             const float* step_coef, const float* x0_coef, const float* known_level, int32_t n_steps,
                             const float* null_cond_host, float guidance_scale, const float* known, int64_t ld_known,
                             const float* lo_host, const float* hi_host) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags, false, timesteps, step_coef, n_steps,
                  null_cond_host != nullptr, null_cond_host, guidance_scale, known != nullptr, known, ld_known, known_level,
                  true, x0_coef, lo_host, hi_host};
  return sample_request(h, r);
}

int osd_sample_chain_multistep(osd_handle* h, const float* cond, int64_t n, const float* x_T, const float* noises, uint64_t seed,
                               int64_t row_offset, float* x_out, float* mut_mask_out, int flags, const int32_t* timesteps,
                               const float* x0_coef, const float* hist_coef, const float* known_level, int32_t n_steps,
                               const float* null_cond_host, float guidance_scale, const float* known, int64_t ld_known,
                               const float* lo_host, const float* hi_host) {
  SampleRequest r{cond, n, x_T, noises, seed, row_offset, x_out, mut_mask_out, flags, true, timesteps, nullptr, n_steps,
                  null_cond_host != nullptr, null_cond_host, guidance_scale, known != nullptr, known, ld_known, known_level,
                  true, x0_coef, lo_host, hi_host, true, hist_coef};
  return sample_request(h, r);
}

int osd_denoiser_forward_guided(osd_handle* h, const float* x, const int32_t* t_index, int32_t t_all, const float* cond, int64_t n,
                                float* eps, int flags, const float* null_cond_host, float guidance_scale) {
  return forward_request(h, ForwardRequest{x, t_index, t_all, cond, n, eps, flags, nullptr, 0, true, null_cond_host, guidance_scale});
}

int osd_sample_engine(osd_handle* h, int64_t n, int flags) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  if (n < 0) return h->last_engine;
  if (h->precision == 1 && !((flags & OSD_F_TRAIN_MODE) && h->cfg.dropout_p > 0.f)) return 0;     // bf16x3: per-layer launches (split.hip)
  return chain_pick_engine(h, n, flags);
}

int osd_mixup(osd_handle* h, const float* data, const float* cond, const float* surv, const int64_t* perm, double lam, int64_t n,
              float* data_out, float* cond_out, float* surv_out) {
  if (!h) { set_error("null handle"); return OSD_EINVAL; }
  OSD_TRY(check_rows(n));
  if (!perm) { set_error("null perm"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  OSD_HIP(launch_mixup3(h->stream, data_out ? data : nullptr, cond_out ? cond : nullptr, surv_out ? surv : nullptr, perm, lam, n, h->arch.D,
                        h->arch.cond_dim, data_out, cond_out, surv_out));
  return OSD_OK;
}

// Per-launch timing of one reverse step with HIP events on the handle's stream (bench.py's
// roofline leg): launch i of the step (0 = input_proj, 1.. = the block halves in execution
// order, last = output_proj + posterior) averaged over `reps` eager steps at t = T/2.
int osd_profile_step(osd_handle* h, const float* cond, int64_t n, int reps, float* ms_out, double* flop_out, int max_entries,
                     int* n_entries) {
  OSD_TRY(check_ready(h));
  OSD_TRY(check_rows(n));
  if (!cond || !ms_out || !flop_out || !n_entries || n <= 0 || reps <= 0) { set_error("bad argument"); return OSD_EINVAL; }
  const Arch& a = h->arch;
  const int n_launch = 2 + 2 * a.n_blocks;
  if (max_entries < n_launch) { set_error("need room for %d entries", n_launch); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  OSD_TRY(ensure_packed(h, s));
  FwdWs ws;
  const int64_t fwd = carve_fwd(a, nullptr, n, false, &ws);
  const int64_t need = fwd + up64(n * a.D);
  OSD_TRY(h->main.arena.reserve(need));
  carve_fwd(a, h->main.arena, n, false, &ws);
  float* x = h->main.arena + fwd;
  OSD_TRY(run_cond(h, s, cond, n, ws));
  OSD_HIP(launch_fill_randn(s, x, a.D, n, a.D, 1, 0, (uint32_t)a.T, TAG_POSTERIOR));
  std::vector<hipEvent_t> evs((size_t)n_launch + 1);
  for (auto& e : evs) OSD_HIP(hipEventCreate(&e));
  std::vector<double> acc((size_t)n_launch, 0.0);
  int rc = OSD_OK;
  for (int r = 0; r < reps + 1 && rc == OSD_OK; ++r) {       // first pass warms up, untimed
    h->prof_events = &evs;
    h->prof_i = 0;
    hipError_t e = hipEventRecord(evs[h->prof_i++], s);
    TrunkIn in{};
    in.x = x; in.ldx = a.D; in.n = n; in.t_imm = a.T / 2;
    if (e == hipSuccess) rc = run_trunk(h, s, ws, in);
    if (rc == OSD_OK && e == hipSuccess) {
      GemmArgs g = output_proj_args(h, ws, n);
      PosteriorArgs ea{};
      ea.bias = h->params[a.pm.out_b]; ea.xin = x; ea.ldx = a.D; ea.xout = x; ea.ldo = a.D; ea.coef = h->d_coef;
      ea.t_imm = a.T / 2; ea.ldzz = a.D; ea.seed = 1; ea.t_first = a.T / 2;
      e = launch_posterior(s, g, ea);
      if (e == hipSuccess) e = hipEventRecord(evs[h->prof_i++], s);
    }
    h->prof_events = nullptr;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error("profile step failed: %s", hipGetErrorString(e)); rc = OSD_EHIP; break; }
    if (r == 0) continue;
    for (int i = 0; i < n_launch; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, evs[i], evs[i + 1]) == hipSuccess) acc[i] += ms;
    }
  }
  h->prof_events = nullptr;
  for (auto& e : evs) { hipError_t x2 = hipEventDestroy(e); (void)x2; }
  if (rc != OSD_OK) return rc;
  for (int i = 0; i < n_launch; ++i) ms_out[i] = (float)(acc[i] / reps);
  flop_out[0] = 2.0 * (double)n * a.D * a.H0;
  for (int i = 0; i < 2 * a.n_blocks; ++i) {
    const LayerDesc& l = a.layers[i];
    flop_out[1 + i] = 2.0 * (double)n * (l.K1 + l.K2) * l.N;
  }
  flop_out[n_launch - 1] = 2.0 * (double)n * a.block_out[a.n_blocks - 1] * a.D;
  *n_entries = n_launch;
  return OSD_OK;
}

// ---- building blocks for the parity tests -----------------------------------------
int osd_op_linear(osd_handle* h, const float* x, const float* w, const float* b, int64_t n, int K, int N, int silu, float* y) {
  if (!h || !x || !w || !y) { set_error("null argument"); return OSD_EINVAL; }
  OSD_TRY(check_rows(n));
  OSD_HIP(hipSetDevice(h->cfg.device));
  if (h->precision == 1 && !silu && n > 0 && K > 0 && N > 0) return split_op_linear(h, x, w, b, n, K, N, y);
  GemmArgs g{};
  g.A = w; g.lda = K; g.B0 = x; g.ldb0 = K; g.K0 = K; g.F = N; g.P = (int)n; g.K = K;
  OSD_HIP(launch_linear(h->stream, g, true, true, b, y, N, silu != 0, false));
  return OSD_OK;
}

int osd_op_linear_gn_silu(osd_handle* h, const float* x, int K1, const float* x2, int K2, const float* w, const float* b,
                          const float* gamma, const float* beta, int64_t n, int N, float* y) {
  if (!h || !x || !w || !b || !gamma || !beta || !y) { set_error("null argument"); return OSD_EINVAL; }
  OSD_TRY(check_rows(n));
  if (N % 8 || !gn_width_supported(N / 8)) { set_error("unsupported GroupNorm width %d", N / 8); return OSD_EUNSUPPORTED; }
  if (K2 > 0 && (!x2 || K1 % 4)) { set_error("second panel needs x2 and K1 %% 4 == 0"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  GemmArgs g{};
  g.A = w; g.lda = K1 + K2; g.B0 = x; g.ldb0 = K1; g.K0 = K1; g.B1 = x2; g.ldb1 = K2; g.F = N; g.P = (int)n; g.K = K1 + K2;
  GnArgs ga{};
  ga.bias = b; ga.gamma = gamma; ga.beta = beta; ga.out = y; ga.ldo = N;
  OSD_HIP(launch_gn_silu(h->stream, g, N / 8, ga));
  return OSD_OK;
}

int osd_op_gemm(osd_handle* h, const float* A, int lda, int a_kc, const float* B, int ldb, int b_kc, int F, int P, int K, float* C,
                int ldc, int accumulate) {
  if (!h || !A || !B || !C) { set_error("null argument"); return OSD_EINVAL; }
  if (F <= 0 || P <= 0 || K <= 0) { set_error("bad extents"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(h->cfg.device));
  GemmArgs g{};
  g.A = A; g.lda = lda; g.B0 = B; g.ldb0 = ldb; g.K0 = K; g.F = F; g.P = P; g.K = K;
  hipError_t e = launch_linear(h->stream, g, a_kc != 0, b_kc != 0, nullptr, C, ldc, false, accumulate != 0);
  if (e == hipErrorInvalidValue) { set_error("layout/accumulate combination not instantiated"); return OSD_EUNSUPPORTED; }
  OSD_HIP(e);
  return OSD_OK;
}

int osd_op_randn(osd_handle* h, float* out, int64_t rows, int cols, uint64_t seed, int64_t row_offset, uint32_t step, uint32_t kind) {
  if (!h || !out) { set_error("null argument"); return OSD_EINVAL; }
  OSD_TRY(check_rows(rows));
  OSD_HIP(hipSetDevice(h->cfg.device));
  const uint32_t tag = kind == 0 ? (uint32_t)TAG_POSTERIOR : kind == 1 ? (uint32_t)TAG_QNOISE : (uint32_t)TAG_USER + (kind & 0xffu);
  OSD_HIP(launch_fill_randn(h->stream, out, cols, rows, cols, seed, (uint32_t)row_offset, step, tag));
  return OSD_OK;
}

}  // extern "C"
