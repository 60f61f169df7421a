// cox_score.hip -- osd_val_cox_score: the univariate Cox screen, one model per column, every column in one call (DESIGN.md section
// 3.32).  Per column c and in double: u = ((double) x - center) * scale, k = |beta| R, e = exp(beta u - k); over the positions p of
// the plan's descending-time order (cox_plan.h) the risk-set sums A0, A1, A2 of e, e u, e u^2 are running sums read at the END of
// p's tie group (Breslow), and the three outputs are sums over the events of terms in A1 / A0 and A2 / A0.
//
// The running sums couple every position to all before it, so one read of X cannot do: a call is TWO reads of X with a scan of
// block totals between them -- cox.hip's discipline (block sums, a scan of the sums, apply), here with the columns as a second axis.
//   1. coxs_pass<.., 1>:  an item is a block of OSD_COXS_ROWS consecutive positions times a slab of COXS_SLAB columns, one wavefront;
//      a lane owns four columns and walks the block's rows (gathered by the plan's order: a whole row segment per load, coalesced) in
//      position order.  It writes the item's totals of e, e u, e u^2 and, when wanted, the block's max |u|.
//   2. coxs_scan:         per column, the totals become exclusive prefixes over the blocks: COXS_PARTS contiguous runs of blocks are
//      added in block order, the runs in run order.
//   3. coxs_pass<.., 2>:  re-reads X with pass 1's arithmetic, carries A0, A1, A2 from the prefix, adds delta_p (beta u - k) and
//      delta_p u at every position and, where a tie group holding d > 0 events ends, d log A0, d A1 / A0, d (A2 / A0 - (A1 / A0)^2).
//      The item's three partial results take the place of its three prefixes: no other item reads those.
//   4. coxs_reduce:       per column, the items' partial results added as in 2; a column with scale 0 gets exact zeros.
// No floating-point atomics, no workgroup waits for another inside a kernel, every sum has one fixed order.  A column's arithmetic is a
// chain over the positions that no other column enters, and the load path only decides which lane holds it: the same column gives the
// same bits in any call that contains it.  beta_dev == NULL takes HAS_BETA = false: no exp, e = 1, A0 = the position count, exact.
#include <math.h>
#include <stdint.h>
#include <mutex>
#include "cox_plan.h"
#include "handle.h"
#include "val_common.h"

namespace osd {
namespace {

constexpr int COXS_ROWS = OSD_COXS_ROWS;
constexpr int COXS_T = 64;               // an item is one wavefront
constexpr int COXS_PER = 4;              // columns of a lane
constexpr int COXS_SLAB = COXS_T * COXS_PER;
constexpr int COXS_U = 4;                // rows of a load group; two groups are in flight
constexpr int COXS_PARTS = 16;           // runs of blocks of the scan and of the reduction
static_assert(COXS_ROWS % COXS_U == 0, "a block is a whole number of load groups");

struct CoxScoreArgs {
  const float* X; const float* center; const float* scale;
  const double* beta; const double* bound;
  const int* order;              // [rows]: the row at position p
  const unsigned char* ev;       // [rows]: the event flag of position p
  const int* gev;                // [rows]: the events of the tie group that ends at p, else 0
  double* tot;                   // [blocks][3][D]: pass 1's totals, then their exclusive prefixes, then pass 2's partial results
  double* bmax;                  // [blocks][D]: the block's max |u|, or null
  long long ld, rows;
  int D;
};

template <bool ALIGNED>
__device__ __forceinline__ int coxs_col(int slab, int lane, int e) {
  return slab * COXS_SLAB + (ALIGNED ? COXS_PER * lane + e : lane + COXS_T * e);
}

// the lane's four values of row `row`; a column beyond D reads as 0
template <bool ALIGNED>
__device__ __forceinline__ void coxs_load(const CoxScoreArgs& a, float (&x)[COXS_PER], long long row, int slab, int lane) {
  const float* p = a.X + (size_t)row * (size_t)a.ld;
  if (ALIGNED) {
    const int q = coxs_col<true>(slab, lane, 0);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < a.D) v = *reinterpret_cast<const float4*>(p + q);      // ld >= roundup(D, 4): inside the row
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < COXS_PER; ++e) {
      const int col = coxs_col<false>(slab, lane, e);
      x[e] = col < a.D ? p[col] : 0.f;
    }
  }
}

// PASS 1: the item's totals.  PASS 2: from the prefixes to the item's partial results.
template <bool HAS_BETA, bool ALIGNED, int PASS>
__global__ __launch_bounds__(COXS_T) void coxs_pass(CoxScoreArgs a) {
  const int lane = threadIdx.x, slab = blockIdx.y;
  const long long blk = blockIdx.x;
  const long long p0 = blk * COXS_ROWS, p1 = min(a.rows, p0 + COXS_ROWS);      // p0 < p1: the host launches no empty block
  double c[COXS_PER], s[COXS_PER], be[COXS_PER], k[COXS_PER];
  double A0[COXS_PER], A1[COXS_PER], A2[COXS_PER];                             // pass 1: the totals; pass 2: the running sums
  double ll[COXS_PER], su[COXS_PER], sm[COXS_PER], inf[COXS_PER], mx[COXS_PER];
  bool in[COXS_PER];
#pragma unroll
  for (int e = 0; e < COXS_PER; ++e) {
    const int col = coxs_col<ALIGNED>(slab, lane, e);
    in[e] = col < a.D;
    c[e] = in[e] ? (double)a.center[col] : 0.0;
    s[e] = in[e] ? (double)a.scale[col] : 0.0;
    be[e] = HAS_BETA && in[e] ? a.beta[col] : 0.0;
    k[e] = HAS_BETA && in[e] && a.bound ? fabs(be[e]) * a.bound[col] : 0.0;
    A0[e] = A1[e] = A2[e] = 0.0;
    if (PASS == 2 && in[e]) {
      const size_t at = (size_t)blk * 3 * (size_t)a.D + (size_t)col;
      if (HAS_BETA) A0[e] = a.tot[at];
      A1[e] = a.tot[at + (size_t)a.D];
      A2[e] = a.tot[at + 2 * (size_t)a.D];
    }
    ll[e] = su[e] = sm[e] = inf[e] = mx[e] = 0.0;
  }
  // Two buffers of COXS_U rows: the loads of the next group are in flight while this group's arithmetic runs.  A position beyond
  // the block re-reads the block's last one and is not used.
  struct Group { float x[COXS_U][COXS_PER]; int ev[COXS_U], gev[COXS_U]; };
  auto fetch = [&](Group& g, long long g0) {
#pragma unroll
    for (int r = 0; r < COXS_U; ++r) {
      const long long p = min(g0 + r, p1 - 1);
      coxs_load<ALIGNED>(a, g.x[r], (long long)a.order[p], slab, lane);
      g.ev[r] = PASS == 2 ? (int)a.ev[p] : 0;
      g.gev[r] = PASS == 2 ? a.gev[p] : 0;
    }
  };
  auto consume = [&](const Group& g, long long g0) {
#pragma unroll
    for (int r = 0; r < COXS_U; ++r) {
      const long long p = g0 + r;
      if (p >= p1) break;                                    // uniform: the whole wavefront leaves together
      const bool event = g.ev[r] != 0;
      const int d = g.gev[r];
#pragma unroll
      for (int e = 0; e < COXS_PER; ++e) {
        const double u = ((double)g.x[r][e] - c[e]) * s[e];
        double t = 0.0, eu = u;
        if (HAS_BETA) {
          t = be[e] * u - k[e];
          const double ex = exp(t);
          A0[e] += ex;
          eu = ex * u;
        }
        A1[e] += eu;
        A2[e] += eu * u;
        if (PASS == 1) mx[e] = fmax(mx[e], fabs(u));
        if (event) {
          su[e] += u;
          if (HAS_BETA) ll[e] += t;
        }
        if (d > 0) {                                         // a tie group with d events ends here: its risk set is complete
          const double a0 = HAS_BETA ? A0[e] : (double)(p + 1), dg = (double)d;
          const double m1 = A1[e] / a0;
          ll[e] -= dg * log(a0);
          sm[e] += dg * m1;
          inf[e] += dg * (A2[e] / a0 - m1 * m1);
        }
      }
    }
  };
  Group ga, gb;
  fetch(ga, p0);
  for (long long g0 = p0; g0 < p1; g0 += 2 * COXS_U) {
    if (g0 + COXS_U < p1) fetch(gb, g0 + COXS_U);
    consume(ga, g0);
    if (g0 + COXS_U >= p1) break;
    if (g0 + 2 * COXS_U < p1) fetch(ga, g0 + 2 * COXS_U);
    consume(gb, g0 + COXS_U);
  }
#pragma unroll
  for (int e = 0; e < COXS_PER; ++e) {
    if (!in[e]) continue;
    const int col = coxs_col<ALIGNED>(slab, lane, e);
    const size_t at = (size_t)blk * 3 * (size_t)a.D + (size_t)col;
    if (PASS == 1) {
      if (HAS_BETA) a.tot[at] = A0[e];
      a.tot[at + (size_t)a.D] = A1[e];
      a.tot[at + 2 * (size_t)a.D] = A2[e];
      if (a.bmax) a.bmax[(size_t)blk * (size_t)a.D + (size_t)col] = mx[e];
    } else {
      a.tot[at] = ll[e];
      a.tot[at + (size_t)a.D] = su[e] - sm[e];
      a.tot[at + 2 * (size_t)a.D] = inf[e];
    }
  }
}

// tot[b][k][col] becomes the sum over the blocks before b, k = k0 + blockIdx.y: wave w owns the w-th run of `chunk` blocks, adds it
// in block order, and starts its prefixes from the runs before it, added in run order
__global__ __launch_bounds__(COXS_T * COXS_PARTS) void coxs_scan(double* __restrict__ tot, long long blocks, long long chunk, int D, int k0) {
  __shared__ double part[COXS_PARTS][COXS_T];
  const int cx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * COXS_T + cx, k = k0 + blockIdx.y;
  const long long b0 = min(blocks, (long long)w * chunk), b1 = min(blocks, b0 + chunk);
  const bool in = col < D;
  double* base = tot + (size_t)k * (size_t)D + (size_t)(in ? col : 0);
  const size_t step = 3 * (size_t)D;
  double sum = 0.0;
  if (in)
    for (long long b = b0; b < b1; ++b) sum += base[(size_t)b * step];
  part[w][cx] = sum;
  __syncthreads();
  if (!in) return;
  double run = 0.0;
  for (int q = 0; q < w; ++q) run += part[q][cx];
  for (long long b = b0; b < b1; ++b) {
    const double v = base[(size_t)b * step];
    base[(size_t)b * step] = run;
    run += v;
  }
}

// out[k][col] = the sum over the blocks of tot[b][k][col], the runs as in coxs_scan; a column with scale 0: exactly 0.
// absmax[col] = the maximum over the blocks of bmax[b][col].
__global__ __launch_bounds__(COXS_T * COXS_PARTS) void coxs_reduce(const double* __restrict__ tot, const double* __restrict__ bmax,
                                                                   long long blocks, long long chunk, int D, const float* __restrict__ scale,
                                                                   double* __restrict__ loglik, double* __restrict__ score,
                                                                   double* __restrict__ info, double* __restrict__ absmax) {
  __shared__ double part[4][COXS_PARTS][COXS_T];
  const int cx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = blockIdx.x * COXS_T + cx;
  const long long b0 = min(blocks, (long long)w * chunk), b1 = min(blocks, b0 + chunk);
  double s[3] = {0.0, 0.0, 0.0}, m = 0.0;
  if (col < D)
    for (long long b = b0; b < b1; ++b) {
      const size_t at = (size_t)b * 3 * (size_t)D + (size_t)col;
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] += tot[at + (size_t)k * (size_t)D];
      if (bmax) m = fmax(m, bmax[(size_t)b * (size_t)D + (size_t)col]);
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) part[k][w][cx] = s[k];
  part[3][w][cx] = m;
  __syncthreads();
  if (w != 0 || col >= D) return;
  for (int q = 1; q < COXS_PARTS; ++q) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += part[k][q][cx];
    m = fmax(m, part[3][q][cx]);
  }
  const bool dropped = scale[col] == 0.f;
  loglik[col] = dropped ? 0.0 : s[0];
  score[col] = dropped ? 0.0 : s[1];
  info[col] = dropped ? 0.0 : s[2];
  if (absmax) absmax[col] = m;
}

// One grow-only workspace per device (cox_plan.h): a screen's Newton iterations call again and again.
CoxWorkspace* const g_coxs_ws = new CoxWorkspace[COX_MAX_DEVICES];  // never destroyed: no hipFree from a static destructor at process exit

template <bool HAS_BETA, int PASS>
hipError_t coxs_launch(bool aligned, dim3 grid, hipStream_t s, const CoxScoreArgs& a) {
  return launched(aligned ? coxs_pass<HAS_BETA, true, PASS> : coxs_pass<HAS_BETA, false, PASS>, grid, dim3(COXS_T), 0, s, a);
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" int osd_val_cox_score(void* plan, const float* X, int64_t rows, int ld, int D, const float* center, const float* scale,
                                 const double* beta_dev, const double* bound_dev, double* loglik_dev, double* score_dev,
                                 double* info_dev, double* absmax_dev) {
  CoxPlan* pl = (CoxPlan*)plan;
  if (!pl || !X || !center || !scale || !loglik_dev || !score_dev || !info_dev || rows < 1 || D < 1 || D > COX_MAX_D || ld < D) {
    set_error("bad argument (a plan, rows >= 1, 1 <= D <= 8192, ld >= D, the three outputs)");
    return OSD_EINVAL;
  }
  if (rows != pl->rows) {
    set_error("the plan was made for %lld rows, not %lld", (long long)pl->rows, (long long)rows);
    return OSD_EINVAL;
  }
  OSD_HIP(hipSetDevice(pl->device));
  hipStream_t s = pl->stream;

  const int Dq = (D + 3) / 4 * 4;
  const bool aligned = (reinterpret_cast<uintptr_t>(X) & 15) == 0 && ld % 4 == 0 && ld >= Dq;
  const long long blocks = (rows + COXS_ROWS - 1) / COXS_ROWS;
  const long long chunk = (blocks + COXS_PARTS - 1) / COXS_PARTS;
  const unsigned slabs = (unsigned)((D + COXS_SLAB - 1) / COXS_SLAB), col_groups = (unsigned)((D + COXS_T - 1) / COXS_T);
  const bool has_beta = beta_dev != nullptr;

  CoxWorkspace& ws = g_coxs_ws[pl->device];
  std::lock_guard<std::mutex> hold(ws.mu);
  const size_t tot_bytes = up256((size_t)blocks * 3 * (size_t)D * sizeof(double));
  const size_t max_bytes = absmax_dev ? up256((size_t)blocks * (size_t)D * sizeof(double)) : 0;
  OSD_TRY(ws.buf.reserve((int64_t)(tot_bytes + max_bytes)));

  CoxScoreArgs a{};
  a.X = X; a.center = center; a.scale = scale; a.beta = beta_dev; a.bound = has_beta ? bound_dev : nullptr;
  a.order = pl->order.get(); a.ev = pl->ev.get(); a.gev = pl->gev.get();
  a.tot = (double*)ws.buf.get();
  a.bmax = absmax_dev ? (double*)(ws.buf.get() + tot_bytes) : nullptr;
  a.ld = ld; a.rows = rows; a.D = D;

  const dim3 grid((unsigned)blocks, slabs);
  OSD_HIP((has_beta ? coxs_launch<true, 1>(aligned, grid, s, a) : coxs_launch<false, 1>(aligned, grid, s, a)));
  // without beta A0 is a count: its plane holds nothing until pass 2 writes the log-likelihood's partial results there
  OSD_HIP(launched(coxs_scan, dim3(col_groups, has_beta ? 3u : 2u), dim3(COXS_T * COXS_PARTS), 0, s, a.tot, blocks, chunk, D,
                   has_beta ? 0 : 1));
  OSD_HIP((has_beta ? coxs_launch<true, 2>(aligned, grid, s, a) : coxs_launch<false, 2>(aligned, grid, s, a)));
  OSD_HIP(launched(coxs_reduce, dim3(col_groups), dim3(COXS_T * COXS_PARTS), 0, s, (const double*)a.tot, (const double*)a.bmax, blocks,
                   chunk, D, scale, loglik_dev, score_dev, info_dev, absmax_dev));
  OSD_HIP(hipStreamSynchronize(s));
  return OSD_OK;
}
