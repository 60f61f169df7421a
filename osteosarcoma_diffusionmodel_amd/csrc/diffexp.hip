// diffexp.hip -- per-feature two-GROUP rank statistics inside one device-resident cohort:
//   osd_val_group_ranks   per feature twice the Mann-Whitney U of the cases over the controls (ties counted 1/2), the tie correction
//                         sum (t^3 - t) of the normal approximation, and each group's first two centred moments.
//
// The labels are read back once and turned into a row -> slot map on the host (case k of the cohort goes to slot k, control k to slot
// na + k, every other row to -1); the columns then go through in chunks, as in marginal.hip, on the shared pieces of val_columns.h
// (the chunked driver's state, the tile transposer, the binary searches, the phase timer).  Per chunk:
//   col_tiles<true>   the [rows, chunk] column slice of the row-major matrix through the 64 x 64 LDS tile; a case row's values land
//                 in the column-major case segments, a control row's in the control segments, an ignored row's nowhere
//   seg_sort      segsort.h's four stable 8-bit passes over the case segments, then over the control segments: sorted in place
//   de_stats      workgroup (x, f) owns elements [x R, (x + 1) R) of BOTH sorted segments of feature f (R = COL_RUN), staged in LDS.
//                 The lower bound of the run's first value and the upper bound of its last one in the OTHER segment enclose every
//                 bound the run can ask for: that window is staged in LDS and searched there (COL_WINDOW floats; a wider window --
//                 heavy ties, groups of very different size -- is searched in global memory between the same two ends).
//                 u2: every case value a_i adds #{b < a_i} + #{b <= a_i}; the second is the first unless b holds a_i (one probe).
//                 ties: a last-of-its-value case element adds t^3 - t with t = its run in a + (upper - lower) in b; a
//                 last-of-its-value control element whose value does not occur in a adds it with t = its run in b.  A run's length
//                 is the element's index + 1 - the lower bound of its value in its own segment: searched in the staged run, and
//                 before the run's start in global memory only for the one value that reaches it.
//                 moments: (double)x - (double)c and its square, summed per lane in index order, over the wavefront by the xor
//                 butterfly, over the four wavefronts in order.
//                 One slot per workgroup for the six sums: no atomic of any kind.
//   de_finish     one wavefront per feature: the slots in a fixed order.
// Every comparison is a float comparison, so -0.0 and +0.0 are one value although the sort keeps them apart.  The partition of a
// feature's elements depends on (na, nb) alone and every sum runs over sorted data: the same bits at every chunk size, on every call
// and for every order of the rows.
#include <stdint.h>
#include <string.h>
#include <vector>
#include <hip/hip_runtime.h>
#include "handle.h"
#include "val_columns.h"

namespace osd {
namespace {

constexpr int64_t DE_MAX_N = 1ll << 20;    // na + nb: up to here ties <= N^3 - N stays under 2^60

struct DeArgs {
  const float* a; const float* b;          // sorted segments [chunk][na], [chunk][nb]
  long long na, nb;
  int blocks;                              // workgroups of a feature: ceil(max(na, nb) / COL_RUN)
  const float* center;                     // the chunk's first column's centre, or NULL
  long long* pu2; long long* pties;        // [chunk][blocks]
  double* psum; double* psq;               // [2][chunk][blocks]: cases, controls
};

// The run [i0, i1) of the sorted segment x (nx values) against the other segment y (ny values); CASE: x is the case segment.
// i0 < i1 <= nx, i1 - i0 <= COL_RUN.  Adds to u2 (CASE only), ties, and the run's centred moments.
template <bool CASE>
__device__ __forceinline__ void de_run(const float* __restrict__ x, long long nx, long long i0, long long i1, const float* __restrict__ y,
                                       long long ny, double c, float* own, float* win, long long* ends, long long& u2, long long& ties,
                                       double& sum, double& sq) {
  const int len = (int)(i1 - i0);
  if (threadIdx.x == 0) ends[0] = lower_bound(y, 0ll, ny, x[i0]);
  if (threadIdx.x == 64) ends[1] = upper_bound(y, 0ll, ny, x[i1 - 1]);
  for (int k = threadIdx.x; k < len; k += COL_THREADS) own[k] = x[i0 + k];
  __syncthreads();
  const long long lo = ends[0], hi = ends[1];                  // lo <= hi: x ascending
  const bool staged = hi - lo <= COL_WINDOW;                   // the same in the whole workgroup
  const int wn = staged ? (int)(hi - lo) : 0;
  for (int k = threadIdx.x; k < wn; k += COL_THREADS) win[k] = y[lo + k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < COL_ITEMS; ++k) {
    const int j = k * COL_THREADS + threadIdx.x;               // index in the run
    if (j >= len) continue;
    const long long i = i0 + j;
    const float v = own[j];
    const double d = (double)v - c;
    sum += d;
    sq += d * d;
    // y[< lo] < x[i0] <= v and y[>= hi] > x[i1 - 1] >= v: both bounds of v lie in [lo, hi]
    // the upper bound is the lower one unless y holds v: one probe spares the second search on untied data
    long long lb, ub;
    if (staged) {
      const int l = lower_bound(win, 0, wn, v);
      lb = lo + l;
      ub = CASE && l < wn && win[l] == v ? lo + upper_bound(win, l + 1, wn, v) : lb;
    } else {
      lb = lower_bound(y, lo, hi, v);
      ub = CASE && lb < hi && y[lb] == v ? upper_bound(y, lb + 1, hi, v) : lb;
    }
    if (CASE) u2 += lb + ub;
    const bool last = j + 1 < len ? own[j + 1] != v : (i + 1 >= nx || x[i + 1] != v);
    if (!last) continue;                                       // a later element carries this value
    if (!CASE && lb < hi && (staged ? win[lb - lo] : y[lb]) == v) continue;      // the case segment counts this value
    long long first = i;
    if (j == 0 || own[j - 1] == v) {
      const int l = lower_bound(own, 0, j, v);
      first = i0 + l;
      if (l == 0 && i0 > 0) first = lower_bound(x, 0ll, i0, v);      // the value reaches the run's start: at most one such element
    }
    const long long t = (i + 1 - first) + (CASE ? ub - lb : 0);
    ties += t * t * t - t;
  }
  __syncthreads();                                             // own, win and ends are free again
}

__global__ __launch_bounds__(COL_THREADS) void de_stats(DeArgs g) {
  __shared__ float win[COL_WINDOW];
  __shared__ float own[COL_RUN];
  __shared__ long long ends[2];
  __shared__ long long ru2[COL_THREADS / 64], rties[COL_THREADS / 64];
  __shared__ double rsum[4][COL_THREADS / 64];
  const long long f = blockIdx.y;
  const float* a = g.a + f * g.na;
  const float* b = g.b + f * g.nb;
  const double c = g.center ? (double)g.center[f] : 0.0;
  const long long i0 = (long long)blockIdx.x * COL_RUN;
  const long long a1 = min(g.na, i0 + COL_RUN), b1 = min(g.nb, i0 + COL_RUN);
  long long u2 = 0, ties = 0;
  double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
  // every condition below is the same in the whole workgroup: the barriers inside de_run are met by all or by none
  if (i0 < g.na) de_run<true>(a, g.na, i0, a1, b, g.nb, c, own, win, ends, u2, ties, sa, qa);
  if (i0 < g.nb) de_run<false>(b, g.nb, i0, b1, a, g.na, c, own, win, ends, u2, ties, sb, qb);
  wave_sum(u2, ties, sa, qa, sb, qb);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { ru2[wv] = u2; rties[wv] = ties; rsum[0][wv] = sa; rsum[1][wv] = qa; rsum[2][wv] = sb; rsum[3][wv] = qb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < COL_THREADS / 64; ++w) {
      u2 += ru2[w]; ties += rties[w];
      sa += rsum[0][w]; qa += rsum[1][w]; sb += rsum[2][w]; qb += rsum[3][w];
    }
    const long long slot = f * g.blocks + blockIdx.x, group = (long long)gridDim.y * g.blocks;
    g.pu2[slot] = u2; g.pties[slot] = ties;
    g.psum[slot] = sa; g.psq[slot] = qa; g.psum[group + slot] = sb; g.psq[group + slot] = qb;
  }
}

// One wavefront per feature.  out: six arrays of `chunk` 8-byte values -- u2, ties (long long), then the cases' and the controls'
// sum and the cases' and the controls' sum of squares (double).  `group`: the slots of one group, as de_stats laid them out.
__global__ __launch_bounds__(64) void de_finish(DeArgs g, int chunk, long long group, long long* out) {
  const int f = blockIdx.x, lane = threadIdx.x;
  long long u2 = 0, ties = 0;
  double sa = 0.0, qa = 0.0, sb = 0.0, qb = 0.0;
  for (int k = lane; k < g.blocks; k += 64) {                   // lane order, then the butterfly: fixed by (na, nb)
    const long long slot = (long long)f * g.blocks + k;
    u2 += g.pu2[slot]; ties += g.pties[slot];
    sa += g.psum[slot]; qa += g.psq[slot]; sb += g.psum[group + slot]; qb += g.psq[group + slot];
  }
  wave_sum(u2, ties, sa, qa, sb, qb);
  if (lane == 0) {
    double* o = (double*)out;
    out[f] = u2;
    out[chunk + f] = ties;
    o[2 * chunk + f] = sa; o[3 * chunk + f] = sb; o[4 * chunk + f] = qa; o[5 * chunk + f] = qb;
  }
}

int group_ranks(void* stream, int device, const float* X, int64_t rows, int ld, int D, const int32_t* labels, const float* center,
                int chunk_cols, int64_t* u2, int64_t* ties, double* sum, double* sumsq, int64_t* na_out, int64_t* nb_out, double* phase_ms) {
  if (!X || !labels || !u2 || !ties || !sum || !sumsq || !na_out || !nb_out) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  if (rows < 1 || D < 1 || ld < D || chunk_cols < 0) {
    set_error("bad argument (rows, D >= 1, ld >= D, chunk_cols >= 0)");
    return OSD_EINVAL;
  }
  if (rows > 2000000000ll) { set_error("too many rows for one gather"); return OSD_EINVAL; }
  OSD_HIP(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;

  // the row -> slot map: the cases in row order, then the controls in row order
  std::vector<int32_t> map((size_t)rows);
  OSD_HIP(read_back(s, map.data(), labels, (size_t)rows * sizeof(int32_t)));
  int64_t na = 0, nb = 0;
  for (int64_t r = 0; r < rows; ++r) { na += map[r] == 1; nb += map[r] == 0; }
  *na_out = na; *nb_out = nb;
  if (na < 1 || nb < 1) { set_error("a group is empty (%lld cases, %lld controls)", (long long)na, (long long)nb); return OSD_EINVAL; }
  if (na + nb > DE_MAX_N) { set_error("more than 2^20 labelled rows: the tie sum could pass 2^60"); return OSD_EINVAL; }
  int64_t ia = 0, ib = na;
  for (int64_t r = 0; r < rows; ++r) map[r] = map[r] == 1 ? (int32_t)ia++ : map[r] == 0 ? (int32_t)ib++ : -1;

  ColumnChunks cc;                                             // init's clamp leaves >= 1: na, nb <= 2^20
  OSD_TRY(cc.init(na, nb, D, chunk_cols ? chunk_cols : osd_val_marginals_auto_chunk(na, nb, D)));
  const int64_t chunk = cc.chunk, blocks = cc.blocks;
  ValBuf slot_of, slots, res;
  OSD_TRY(slot_of.alloc((size_t)rows * sizeof(int32_t)));
  OSD_TRY(slots.alloc((size_t)(6 * chunk * blocks) * 8));
  OSD_TRY(res.alloc((size_t)(6 * chunk) * 8));
  OSD_HIP(hipMemcpyAsync(slot_of.get(), map.data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, s));
  DeArgs g{};
  g.a = cc.ca; g.b = cc.cb; g.na = na; g.nb = nb; g.blocks = (int)blocks;
  std::vector<long long> host((size_t)(6 * chunk));
  PhaseClock<3, double> clock(phase_ms);                       // gather, sort, statistics: summed over the chunks
  OSD_HIP(clock.init());

  for (int64_t c0 = 0; c0 < D; c0 += chunk) {
    const int c = (int)(D - c0 < chunk ? D - c0 : chunk);
    const long long group = (long long)c * blocks;             // the slots of one group in this chunk
    g.center = center ? center + c0 : nullptr;
    g.pu2 = slots.as<long long>(); g.pties = g.pu2 + group;
    g.psum = (double*)(g.pties + group); g.psq = g.psum + 2 * group;
    OSD_HIP(clock.mark(0, s));
    OSD_HIP(launched(col_tiles<true>, dim3((unsigned)((rows + COL_TILE - 1) / COL_TILE), (unsigned)((c + COL_TILE - 1) / COL_TILE)), COL_THREADS, 0,
                     s, X + c0, (long long)ld, (long long)rows, c, (const int*)slot_of.as<int>(), (long long)na, (long long)nb, cc.ca, cc.cb));
    OSD_HIP(clock.mark(1, s));
    OSD_TRY(cc.sort(s, c));
    OSD_HIP(clock.mark(2, s));
    OSD_HIP(launched(de_stats, dim3((unsigned)blocks, (unsigned)c), COL_THREADS, 0, s, g));
    OSD_HIP(launched(de_finish, dim3((unsigned)c), 64, 0, s, g, (int)chunk, group, res.as<long long>()));
    OSD_HIP(clock.mark(3, s));
    OSD_HIP(read_back(s, host.data(), res.get(), (size_t)(6 * chunk) * 8));
    OSD_HIP(clock.add());
    for (int f = 0; f < c; ++f) {
      u2[c0 + f] = host[f];
      ties[c0 + f] = host[chunk + f];
      memcpy(&sum[c0 + f], &host[2 * chunk + f], sizeof(double));
      memcpy(&sum[D + c0 + f], &host[3 * chunk + f], sizeof(double));
      memcpy(&sumsq[c0 + f], &host[4 * chunk + f], sizeof(double));
      memcpy(&sumsq[D + c0 + f], &host[5 * chunk + f], sizeof(double));
    }
  }
  return OSD_OK;
}

}  // namespace
}  // namespace osd

using namespace osd;

extern "C" {

int osd_val_group_ranks(void* stream, int device, const float* X, int64_t rows, int ld, int D, const int32_t* labels, const float* center,
                        int chunk_cols, int64_t* u2, int64_t* ties, double* sum, double* sumsq, int64_t* na, int64_t* nb) {
  return group_ranks(stream, device, X, rows, ld, D, labels, center, chunk_cols, u2, ties, sum, sumsq, na, nb, nullptr);
}

int osd_val_group_ranks_timed(void* stream, int device, const float* X, int64_t rows, int ld, int D, const int32_t* labels,
                              const float* center, int chunk_cols, int64_t* u2, int64_t* ties, double* sum, double* sumsq, int64_t* na,
                              int64_t* nb, double* phase_ms) {
  if (!phase_ms) { set_error("bad argument (NULL pointer)"); return OSD_EINVAL; }
  return group_ranks(stream, device, X, rows, ld, D, labels, center, chunk_cols, u2, ties, sum, sumsq, na, nb, phase_ms);
}

}  // extern "C"
