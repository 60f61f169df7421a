// chain.hip -- host side of the persistent reverse-chain kernel (chain.h): eligibility, workspace, launch, status.
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include <algorithm>
#include <vector>
#include "chain.h"
#include "handle.h"
#include "kernels.h"
#include "fwd.h"

namespace osd {

// The chain kernel covers the 128 x 128 tile with GroupNorm groups of 32 or 64 channels (block widths 256 / 512, the
// BASELINE shape and its neighbours) in eval mode; everything else runs on the per-layer kernels.
bool chain_supported(const Arch& a) {
  if (a.H0 % 4) return false;              // D % 4 != 0 runs on the padded chain state (handle.h: Dp)
  for (int c : a.block_out)
    if (c != 256 && c != 512) return false;
  if (a.H0 != 256 && a.H0 != 512) return false;
  if ((int)a.layers.size() + 2 > CHAIN_MAX_LAYERS) return false;
  for (const LayerDesc& l : a.layers)
    if (l.K1 % BK || (l.K1 + l.K2) % BK) return false;        // panel switch on a K-step boundary, no K tail (block weights are not padded)
  return true;
}

int kernel_slots(KernelSlots* cache, int device, const void* kernel, const void* kernel_diag, int threads, int lds_bytes, int cap, int* max_grid) {
  if (device < 0 || device >= 16) { set_error("device %d out of range", device); return OSD_EINVAL; }
  KernelSlots& d = cache[device];
  if (!d.ready) {
    OSD_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    if (kernel_diag) OSD_HIP(hipFuncSetAttribute(kernel_diag, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    int occ = 0;
    OSD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds_bytes));
    hipDeviceProp_t prop;
    OSD_HIP(hipGetDeviceProperties(&prop, device));
    d.occ = std::min(occ, cap);
    d.cus = prop.multiProcessorCount;
    d.ready = true;
  }
  *max_grid = d.occ * d.cus;
  return OSD_OK;
}

static int chain_device_limits(int device, int* max_grid) {
  static KernelSlots cache[16];
#ifdef OSD_DIAG
  const void* diag = reinterpret_cast<const void*>(chain_kernel<true>);
#else
  const void* diag = nullptr;
#endif
  return kernel_slots(cache, device, reinterpret_cast<const void*>(chain_kernel<false>), diag, NTHREADS, CHAIN_LDS_BYTES,
                      CHAIN_WPS /* two 64 KB tiles per CU by design */, max_grid);
}

// Which chain kernel.  Measured on MI355X (tools/probes/engine_sizes.py, D = 2000, T = 200, M patient-steps/s):
//   rows      per-layer   workspace chain   LDS-resident chain
//    8 192      17.8           5.0               11.4
//   10 240      13.9           6.3               14.3
//   12 288      16.2           7.6               17.1
//   16 384      20.1           9.9               22.5
//   20 480      16.4          12.3               22.6
//   28 672      19.6          17.1               22.3
//   32 768      21.7          19.5               22.4
//   49 152      21.9          19.7               22.4
//   65 536      22.2          22.5               22.4
//   81 920      22.3          23.0               22.4
//   98 304      22.5          23.0               22.4
// The LDS-resident kernel (chain_panel.h) runs at 22.4 M from 16 384 rows on -- 64-row units keep every CU busy and its queue has
// no step boundary -- where the per-layer kernels are fast only at whole rounds of their 128 x 128 tiles (multiples of 16 384
// rows) and the workspace chain needs a 128-row tile for each of its 512 slots; from there on the workspace chain leads by
// 1-2.5 % (two independent workgroups per CU hide each other's epilogues).  auto: workspace chain from
// 512 tiles on, LDS-resident chain from 5/8 of the CUs' worth of units (10 240 rows), per-layer kernels below.
static bool panel_window(osd_handle* h, int64_t n) {
  if (!panel_chain_supported(h)) return false;
  const int slots = panel_chain_slots(h);
  if (slots < 1) return false;
  const int64_t units = (n + 63) / 64;
  return units * 8 >= (int64_t)slots * 5;
}

static bool chain_use_panel(osd_handle* h, int64_t n) {
  if (h->chain_variant == 1) return false;
  if (h->chain_variant == 2) return panel_chain_supported(h);
  int max_grid = 0;
  if (chain_device_limits(h->cfg.device, &max_grid) != OSD_OK) return false;
  if ((n + ChainTile::BP - 1) / ChainTile::BP >= (int64_t)max_grid) return false;       // the workspace chain has a tile per slot
  return panel_window(h, n);
}

// The squad chain: asked for by name, or auto's choice for a small batch in the small-batch mode (osd_set_option("input_splitk",
// != 0): the switch that already trades "results do not depend on the batch size, bit for bit" for latency; the library default
// keeps that invariance, utils/generate.py's front end turns the mode on).  An explicit sampler = chain keeps the kernels that
// are bit-identical to the per-layer engine.
bool chain_uses_squad(osd_handle* h, int64_t n) {
  if (!squad_window(h, n)) return false;
  return h->chain_variant == 3 || (h->sampler == 0 && h->input_splitk != 0 && !h->splitk_suspended);
}

// 0 = per-layer kernels (eager or hipGraph), 1 = persistent chain kernel
int chain_pick_engine(osd_handle* h, int64_t n, int flags) {
  if (h->sampler == 2) return 0;
  if ((flags & OSD_F_TRAIN_MODE) && h->cfg.dropout_p > 0.f) return 0;       // dropout inside the chain: per-layer kernels
  if (!chain_supported(h->arch)) return 0;
  if (h->sampler == 1) return 1;
  int max_grid = 0;
  if (chain_device_limits(h->cfg.device, &max_grid) != OSD_OK || max_grid < 2) return 0;
  const int64_t n_tiles = (n + ChainTile::BP - 1) / ChainTile::BP;
  // every slot gets a tile: with fewer tiles than resident workgroups the workspace chain idles CUs (384 tiles: 19.4 M
  // patient-steps/s against 21.8 M for the per-layer engine, which also tiles the features; 512 tiles: 22.2 vs 22.1; beyond
  // that the chain kernel leads -- tools/probes/engine_crossover.py); below that, the LDS-resident chain where it leads
  if (n_tiles >= (int64_t)max_grid) return 1;
  if (h->chain_variant != 1 && h->chain_variant != 3 && panel_window(h, n)) return 1;
  // small batches (the reference's own generation sizes) in the small-batch mode: every 32-patient squad of the chain resident at once
  if (chain_uses_squad(h, n)) return 1;
  return 0;
}

// sync words: [status, queue, pad x2 | cu arrivals x2048 | progress x n_tiles], zeroed before every chain
int chain_ensure_sync(osd_handle* h, int64_t n_tiles, hipStream_t s) {
  const int64_t words = 4 + 2048 + ((n_tiles + 3) / 4) * 4;
  OSD_TRY(h->chain_sync.reserve(words, s));
  OSD_HIP(hipMemsetAsync(h->chain_sync, 0, (size_t)words * 4, s));
  return OSD_OK;
}

// Waits for the chain launched last and reads its status word into *st.  The wait is a hipStreamQuery poll with a wall-clock
// budget (10 x the estimated run time + 2 s, or osd_set_option("chain_wall_budget_ms")): the in-kernel spin budget cannot see a
// workgroup that is stuck at a barrier, and a blind hipStreamSynchronize would then block the caller forever.  On expiry the
// host raises CHAIN_ABORT in the status word through a second stream -- every dependency wait and every unit boundary checks
// that word, so a kernel whose workgroups are merely waiting drains within microseconds -- and gives the device a grace period;
// OSD_EHIP only if the kernel still does not end (the stream is then unusable and the message says so).
static int chain_wait_status(osd_handle* h, unsigned* st) {
  *st = CHAIN_OK;
  if (!h->chain_pending || !h->chain_sync) return OSD_OK;
  hipStream_t s = h->stream;
  const double budget_ms = h->chain_wall_budget_ms > 0 ? (double)h->chain_wall_budget_ms : 10.0 * h->chain_expected_ms + 2000.0;
  auto now_ms = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec; };
  auto poll = [&](double limit_ms) -> hipError_t {
    const double t0 = now_ms();
    for (;;) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return e;
      const double el = now_ms() - t0;
      if (el > limit_ms) return hipErrorNotReady;
      if (el > 2.0) usleep(el > 100.0 ? 1000 : 100);      // short chains: spin; long ones: sleep between polls
    }
  };
  hipError_t e = poll(budget_ms);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();
    if (!h->abort_stream) OSD_HIP(hipStreamCreateWithFlags(h->abort_stream.put(), hipStreamNonBlocking));
    static const unsigned abort_word = CHAIN_ABORT;
    OSD_HIP(hipMemcpyAsync(h->chain_sync, &abort_word, 4, hipMemcpyHostToDevice, h->abort_stream));
    OSD_HIP(hipStreamSynchronize(h->abort_stream));
    e = poll(std::max(5000.0, 0.25 * budget_ms));
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      set_error("the reverse-chain kernel did not finish within %.0f ms and did not react to the abort flag (a workgroup is stuck outside a "
                "dependency wait); the handle's stream is blocked -- destroy the process's HIP context", budget_ms);
      return OSD_EHIP;
    }
  }
  OSD_HIP(e);
  OSD_HIP(hipMemcpyAsync(st, h->chain_sync, 4, hipMemcpyDeviceToHost, s));
  OSD_HIP(hipStreamSynchronize(s));
  h->chain_pending = false;
  return OSD_OK;
}

// Blocks until the previous chain's status word is known; OSD_EHIP if that chain gave up in a dependency wait.
int chain_check_status(osd_handle* h) {
  unsigned st = CHAIN_OK;
  OSD_TRY(chain_wait_status(h, &st));
  if (st != CHAIN_OK) {
    set_error("the reverse-chain kernel gave up waiting for a row tile of an earlier step (status %u: %s): its results are invalid; "
              "call osd_sample_chain with OSD_F_SYNC to have such a chain re-run on the per-layer kernels, or osd_set_option(\"sampler\", 2)",
              st, st == CHAIN_ABORT ? "host wall-clock budget" : "in-kernel spin budget");
    return OSD_EHIP;
  }
  return OSD_OK;
}

// Synchronous variant for osd_sample_chain(OSD_F_SYNC): *gave_up = 1 when the chain's results are invalid (the caller re-runs
// the chain on the per-layer kernels), errors only for HIP failures and a device that does not come back.
int chain_finish(osd_handle* h, int* gave_up) {
  unsigned st = CHAIN_OK;
  OSD_TRY(chain_wait_status(h, &st));
  *gave_up = st != CHAIN_OK;
  return OSD_OK;
}

// ---- host skeleton common to the three chain kernels ----
int chain_hoist_cond(osd_handle* h, hipStream_t s, const float* cond, int64_t n, int64_t rows_pad, FwdWs* cw) {
  const int H0 = h->arch.H0;
  const int64_t c_off_ce2 = up64(n * 64), c_off_cp = c_off_ce2 + up64(n * 64);
  OSD_TRY(h->chain_cond.reserve(c_off_cp + up64(rows_pad * H0), s));
  cw->ce1 = h->chain_cond; cw->ce2 = h->chain_cond + c_off_ce2; cw->cproj = h->chain_cond + c_off_cp;
  OSD_TRY(run_cond(h, s, cond, n, *cw));
  if (rows_pad > n) OSD_HIP(hipMemsetAsync(cw->cproj + n * H0, 0, (size_t)(rows_pad - n) * H0 * 4, s));
  return OSD_OK;
}

int chain_state(osd_handle* h, hipStream_t s, const ChainJob& job, int state_cols, float** xs) {
  const int64_t n = job.n;
  *xs = job.x_out;
  if (state_cols != job.D) {
    OSD_TRY(h->chain_xpad.reserve(n * (int64_t)state_cols, s));
    *xs = h->chain_xpad;
    OSD_HIP(hipMemsetAsync(*xs, 0, (size_t)n * state_cols * 4, s));
  }
  return chain_init_state(h, s, job, *xs, state_cols, false);
}

int chain_state_out(hipStream_t s, const ChainJob& job, int state_cols, const float* xs) {
  if (state_cols != job.D) OSD_HIP(launch_copy2d(s, xs, state_cols, job.x_out, job.D, job.n, job.D));
  return OSD_OK;
}

int chain_args_ring(osd_handle* h, hipStream_t s, int S, size_t bytes) {
  OSD_HIP(hipStreamSynchronize(s));        // the host copies are about to be rewritten: earlier uploads must have been consumed
  const int seg = chain_segment_steps(h, S);
  const size_t need = (size_t)((S + seg - 1) / seg) * bytes;
  if (h->chain_args_host.size() < need) h->chain_args_host.resize(need);
  return h->chain_args_dev.reserve((int64_t)need);
}

int chain_args_upload(osd_handle* h, hipStream_t s, int l, const void* args, size_t bytes, const void** dev) {
  char* const host = h->chain_args_host.data() + (size_t)l * bytes;
  *dev = h->chain_args_dev + (size_t)l * bytes;
  memcpy(host, args, bytes);
  OSD_HIP(hipMemcpyAsync(const_cast<void*>(*dev), host, bytes, hipMemcpyHostToDevice, s));
  return OSD_OK;
}

double chain_rounds(int64_t n_tiles, int S, int grid) {
  const double rounds = (double)((n_tiles * S + grid - 1) / grid);
  return grid >= n_tiles ? std::max(rounds, (double)S) : rounds;
}

void chain_launched(osd_handle* h, double expected_ms) {
  h->chain_pending = true;
  h->chain_expected_ms = expected_ms;
}

int chain_run(osd_handle* h, const ChainJob& job) {
  const Arch& a = h->arch;
  const int S = job.plan.n_steps, H0 = a.H0;
  const int64_t n = job.n;
  hipStream_t s = h->stream;
  OSD_TRY(chain_check_status(h));
  if (chain_uses_squad(h, n)) {
    h->last_chain_variant = 3;
    return squad_chain_run(h, job);
  }
  if (chain_use_panel(h, n)) {
    h->last_chain_variant = 2;
    return panel_chain_run(h, job);
  }
  h->last_chain_variant = 1;
  // D % 4 != 0: the kernel works on an internal copy of the state with rows of Dp = roundup(D, 4) floats (pad columns start at
  // zero, meet zero weights in input_proj and get zero eps from the packed output_proj) and the result is copied out at the end
  const bool padded = h->w_out_packed != nullptr;
  if (padded && job.noises) { set_error("internal: injected draws with D %% 4 != 0 run on the per-layer kernels"); return OSD_EUNSUPPORTED; }
  const int D = padded ? h->Dp : a.D;
  int max_grid = 0;
  OSD_TRY(chain_device_limits(h->cfg.device, &max_grid));
  if (max_grid < 1) { set_error("the chain kernel does not fit this device"); return OSD_EUNSUPPORTED; }
  const int BP = ChainTile::BP;
  const int n_tiles = (int)((n + BP - 1) / BP);
  // chain_grid > 0 sets the workgroup count (tests): below the tile count it forces every hand-off across workgroups, above it
  // the surplus workgroups start on later steps of a tile and wait for the earlier ones
  int grid = std::min(n_tiles, max_grid);
  if (h->chain_grid > 0) grid = (int)std::min<int64_t>(std::min(h->chain_grid, max_grid), (int64_t)n_tiles * S);

  // ---- per-slot activation workspace.  Buffers: h0, and (mid, out) of every block, each [128][C]; a buffer is live from the
  // layer that writes it to the last layer that reads it (block outputs of the encoder live on until their decoder block pops
  // them), and dead buffers are reused first-fit: 0.9 MB per slot instead of 1.9 MB at the BASELINE shape, which is what the
  // 512 slots keep cycling through L2 / Infinity Cache ----
  ChainArgs ca{};
  const int nbuf = 1 + 2 * a.n_blocks;                 // 0: h0, 1 + 2b: mid[b], 2 + 2b: out[b]
  std::vector<int> width(nbuf), def(nbuf), last(nbuf);
  width[0] = H0; def[0] = 0; last[0] = 1;              // layer index: 0 input_proj, 1 + 2b / 2 + 2b the halves of block b, 1 + 2 n_blocks output_proj
  for (int b = 0; b < a.n_blocks; ++b) {
    width[1 + 2 * b] = a.block_out[b]; def[1 + 2 * b] = 1 + 2 * b; last[1 + 2 * b] = 2 + 2 * b;
    width[2 + 2 * b] = a.block_out[b]; def[2 + 2 * b] = 2 + 2 * b; last[2 + 2 * b] = 3 + 2 * b;     // next block's first half, or output_proj
    if (a.layers[2 * b].K2 > 0) last[2 + 2 * a.skip_of(b)] = std::max(last[2 + 2 * a.skip_of(b)], 1 + 2 * b);
  }
  std::vector<int64_t> boff(nbuf, -1);
  int64_t off = 0;
  {
    struct Seg { int64_t off, len; int free_from; };    // free_from: first layer index that may overwrite it
    std::vector<Seg> segs;
    for (int i = 0; i < nbuf; ++i) {                     // buffers are defined in increasing layer order
      const int64_t need = up64((int64_t)BP * width[i]);
      int pick = -1;
      for (int sgi = 0; sgi < (int)segs.size(); ++sgi)
        if (segs[sgi].free_from <= def[i] && segs[sgi].len >= need && (pick < 0 || segs[sgi].len < segs[pick].len)) pick = sgi;
      if (pick < 0) { segs.push_back({off, need, 0}); pick = (int)segs.size() - 1; off += need; }
      boff[i] = segs[pick].off;
      // a layer reads its inputs while it writes its output: the segment is reusable by layers AFTER the last reader
      segs[pick].free_from = last[i] + 1;
    }
  }
  const int o_h0 = (int)boff[0];
  std::vector<int> o_mid(a.n_blocks), o_out(a.n_blocks);
  for (int b = 0; b < a.n_blocks; ++b) { o_mid[b] = (int)boff[1 + 2 * b]; o_out[b] = (int)boff[2 + 2 * b]; }
  ca.ws_stride = off;
  OSD_TRY(h->chain_ws.reserve((int64_t)max_grid * off, s));
  ca.ws = h->chain_ws;

  FwdWs cw;
  OSD_TRY(chain_hoist_cond(h, s, job.cond, n, (int64_t)n_tiles * BP, &cw));
  float* xs = nullptr;
  OSD_TRY(chain_state(h, s, job, D, &xs));

  OSD_TRY(chain_ensure_sync(h, n_tiles, s));
  ca.status = h->chain_sync;
  ca.queue = h->chain_sync + 1;
  ca.cu_arrivals = h->chain_stagger > 0 ? h->chain_sync + 4 : nullptr;
  ca.progress = h->chain_sync + 4 + 2048;
  ca.stagger = h->chain_stagger;
  ca.stamps = h->chain_stamps;
  ca.spin_budget = h->chain_spin_budget;    // default 5 s of s_memrealtime ticks: a unit takes milliseconds

  // ---- layer table ----
  const ParamMap& pm = a.pm;
  int nl = 0;
  {
    ChainLayer& L = ca.L[nl++];
    L.A = h->w_in_packed; L.lda = h->w_in_ld; L.K = D; L.K0 = D; L.F = H0;
    L.in0 = -1; L.ld0 = D; L.in1 = 0; L.ld1 = 0; L.out = o_h0; L.ldo = H0; L.kind = CK_INPUT;
    L.bias = h->params[pm.in_b]; L.gamma = nullptr; L.beta = nullptr;
  }
  int cur = o_h0, cur_w = H0;
  for (int b = 0; b < a.n_blocks; ++b) {
    const LayerDesc& l1 = a.layers[2 * b];
    const LayerDesc& l2 = a.layers[2 * b + 1];
    ChainLayer& A1 = ca.L[nl++];
    A1.A = h->params[l1.w]; A1.lda = l1.K1 + l1.K2; A1.K = l1.K1 + l1.K2; A1.K0 = l1.K2 > 0 ? l1.K1 : l1.K1 + l1.K2; A1.F = l1.N;
    A1.in0 = cur; A1.ld0 = cur_w; A1.in1 = 0; A1.ld1 = 0;
    if (l1.K2 > 0) { A1.in1 = o_out[a.skip_of(b)]; A1.ld1 = a.block_out[a.skip_of(b)]; }
    A1.out = o_mid[b]; A1.ldo = l1.N; A1.kind = l1.gw == 64 ? CK_GN64 : CK_GN32;
    A1.bias = h->params[l1.b]; A1.gamma = h->params[l1.gamma]; A1.beta = h->params[l1.beta];
    ChainLayer& A2 = ca.L[nl++];
    A2.A = h->params[l2.w]; A2.lda = l2.K1; A2.K = l2.K1; A2.K0 = l2.K1; A2.F = l2.N;
    A2.in0 = o_mid[b]; A2.ld0 = l1.N; A2.in1 = 0; A2.ld1 = 0;
    A2.out = o_out[b]; A2.ldo = l2.N; A2.kind = l2.gw == 64 ? CK_GN64 : CK_GN32;
    A2.bias = h->params[l2.b]; A2.gamma = h->params[l2.gamma]; A2.beta = h->params[l2.beta];
    cur = o_out[b]; cur_w = l2.N;
  }
  {
    ChainLayer& L = ca.L[nl++];
    L.A = padded ? h->w_out_packed : h->params[pm.out_w]; L.lda = cur_w; L.K = cur_w; L.K0 = cur_w; L.F = D;
    L.in0 = cur; L.ld0 = cur_w; L.in1 = 0; L.ld1 = 0; L.out = 0; L.ldo = 0; L.kind = CK_POST;
    L.bias = padded ? h->b_out_packed : h->params[pm.out_b]; L.gamma = nullptr; L.beta = nullptr;
  }
  ca.n_layers = nl;
  ca.n_tiles = n_tiles;
  chain_fill_request(ca, h, job, xs, D, cw.cproj);

  // ---- launches: the whole chain in one, or segments of chain_steps_per_launch steps (progress carries over) ----
  OSD_TRY(chain_args_ring(h, s, S, sizeof(ChainArgs)));
  OSD_TRY(for_each_segment(h, S, [&](int launch, int done, int n_steps) -> int {
    ca.t_first = S - 1 - done;
    ca.n_steps = n_steps;
    ca.base_done = (unsigned)done;
    if (done > 0) {                       // per-launch words: the unit queue and the CU arrival counters (status and progress carry over)
      OSD_HIP(hipMemsetAsync(ca.queue, 0, 4, s));
      if (ca.cu_arrivals) OSD_HIP(hipMemsetAsync(ca.cu_arrivals, 0, 2048 * 4, s));
    }
    const void* dev = nullptr;
    OSD_TRY(chain_args_upload(h, s, launch, &ca, sizeof(ChainArgs), &dev));
    const ChainArgs* dargs = static_cast<const ChainArgs*>(dev);
#ifdef OSD_DIAG
    if (ca.stamps) hipLaunchKernelGGL(chain_kernel<true>, dim3(grid), dim3(NTHREADS), CHAIN_LDS_BYTES, s, dargs);
    else
#endif
    hipLaunchKernelGGL(chain_kernel<false>, dim3(grid), dim3(NTHREADS), CHAIN_LDS_BYTES, s, dargs);
    OSD_HIP(hipGetLastError());
    return OSD_OK;
  }));
  OSD_TRY(chain_state_out(s, job, D, xs));
  // run-time estimate for the host's wall-clock budget: a unit (128 rows through every layer) runs at ~0.24 TFLOP/s per
  // resident workgroup when two share a CU (2.8 ms at the BASELINE shape)
  double flop_row = 0;
  for (int l = 0; l < nl; ++l) flop_row += 2.0 * ca.L[l].K * ca.L[l].F;
  chain_launched(h, chain_rounds(n_tiles, S, grid) * (128.0 * flop_row / 0.237e12 * 1e3));
  return OSD_OK;
}


}  // namespace osd
